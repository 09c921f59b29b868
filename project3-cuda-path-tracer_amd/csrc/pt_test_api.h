// pt_test_api.h -- the entry points of include/pt_amd_test.h (device primitives one by one over host arrays, the soundness sweeps of the
// certificates, the fault-word hook, the instrumented builds' read-outs).  They exist only in libpt_amd_test.so (-DPT_TEST_API), the second
// link target of pt_api.hip, which includes this file inside its extern "C" block; the product library exports none of them.
#pragma once

// ---- diagnostics of a renderer (this library's own instance: the product exports none) ----------------------
int pt_debug_trace_paths(int iter, int bounces, float *origin3, float *dir3, float *color3, int32_t *pixelIndex,
                         int32_t *count) {
    if (!R().init) return fail(PT_ERR_NOT_INIT, "pt_debug_trace_paths before pt_init");
    if (bounces < 0 || bounces > PT_MAX_DEPTH || !count) return fail(PT_ERR_INVALID, "pt_debug_trace_paths: bad argument");
    if (bounces > R().prm.traceDepth) return fail(PT_ERR_INVALID, "pt_debug_trace_paths: bounces > traceDepth");
    int rc = sync_all();
    if (rc) return rc;
    if (iter >= 1) activate_step(R(), motion_step(iter));      // (PT_FLAG_MOTION: the iteration's pose; else nothing)
    Slot &sl = R().slot[0];
    if (bounces == 0) {   // camera rays only (they never exist in HBM: generation is fused into bounce 1)
        const int nl = R().nLocal;
        *count = nl;
        if (nl == 0) return PT_OK;
        DevBuf<float> o, d;
        DevBuf<int> px;
        if ((rc = o.alloc((size_t)nl * 3)) || (rc = d.alloc((size_t)nl * 3)) || (rc = px.alloc(nl))) return rc;
        hipLaunchKernelGGL(k_debug_camera_rays, dim3((nl + kBlock - 1) / kBlock), dim3(kBlock), 0, sl.stream, R().prm, iter,
                           o.p, d.p, px.p);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(sl.stream));
        if (origin3) HIPCHECK(hipMemcpy(origin3, o.p, (size_t)nl * 12, hipMemcpyDeviceToHost));
        if (dir3) HIPCHECK(hipMemcpy(dir3, d.p, (size_t)nl * 12, hipMemcpyDeviceToHost));
        if (pixelIndex) HIPCHECK(hipMemcpy(pixelIndex, px.p, (size_t)nl * 4, hipMemcpyDeviceToHost));
        if (color3)
            for (size_t i = 0; i < (size_t)nl * 3; ++i) color3[i] = 1.0f;
        return PT_OK;
    }
    // private run on slot 0: re-arm its cursors, trace, read the queue entering bounce `bounces + 1`, re-arm again
    uint32_t err = 0;
    HIPCHECK(hipMemcpy(&err, &sl.ctrl.p->error, sizeof err, hipMemcpyDeviceToHost));
    rc = reset_ctrl(sl.ctrl.p, sl.stream);
    if (rc) return rc;
    for (int d = 1; d <= bounces; ++d) {
        rc = launch_bounce(sl, iter, 1, d, false, nullptr);  // no radiance, survivors always written
        if (rc) return rc;
    }
    HIPCHECK(hipStreamSynchronize(sl.stream));
    // gather the kSeg segments (chunk lists) of that queue, then sort by pixel index
    static Ctrl h;
    HIPCHECK(hipMemcpy(&h, sl.ctrl.p, sizeof h, hipMemcpyDeviceToHost));
    rc = reset_ctrl(sl.ctrl.p, sl.stream);
    if (rc) return rc;
    err |= h.error;
    if (err) HIPCHECK(hipMemcpy(&sl.ctrl.p->error, &err, sizeof err, hipMemcpyHostToDevice));
    if (h.error) return fail(PT_ERR_DEVICE, "pt_debug_trace_paths: device fault 0x%x", h.error);
    const PathPool pb = pool(sl, bounces & 1);
    const uint32_t gen = sl.gen[bounces & 1];
    std::vector<unsigned long long> lists((size_t)kSeg * R().poolChunks);
    HIPCHECK(hipMemcpy(lists.data(), pb.list, lists.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    uint32_t segn[kSeg];
    size_t n = 0;
    for (int sg = 0; sg < kSeg; ++sg) {
        segn[sg] = h.pos[sl.parity][bounces + 1][sg][0];
        n += segn[sg];
    }
    *count = (int32_t)n;
    if (n == 0) return PT_OK;
    const uint32_t chunkPaths = 1u << R().prm.chunkShift;
    // the pool's three arrays (A: 16 B, B: 16 B, C: 12 B per path), chunk by chunk, into the eleven columns
    std::vector<float> cols[kNumArrays];
    for (int k = 0; k < kNumArrays; ++k) cols[k].resize(n);
    // A history-coded pool (ptk::PathPool; B: {direction.yz, hist, pk}, no array C) comes back as the same eleven columns: the
    // throughput is rebuilt here from `hist` -- `bounces` codes, low end first -- and the material table, by the ordered fp32 products the
    // emitter hit takes (this file is compiled with -ffp-contract=off; products only: nothing to contract either way).
    const int hb = R().prm.histBits;
    std::vector<MaterialDev> hmat;
    if (hb != 0) {
        if (hb * bounces > 32)
            return fail(PT_ERR_INVALID, "pt_debug_trace_paths: %d codes of %d bits do not fit a path's history word (the renderer itself scatters %d times)",
                        bounces, hb, R().prm.traceDepth - 1);
        hmat.resize((size_t)R().prm.nmats);
        HIPCHECK(hipMemcpy(hmat.data(), R().tab.dmats.p, hmat.size() * sizeof(MaterialDev), hipMemcpyDeviceToHost));
    }
    {
        std::vector<float> bufA((size_t)chunkPaths * 4), bufB((size_t)chunkPaths * 4), bufC((size_t)chunkPaths * 3);
        size_t off = 0;
        for (int sg = 0; sg < kSeg; ++sg)
            for (uint32_t done = 0, j = 0; done < segn[sg]; done += chunkPaths, ++j) {
                const uint32_t m = std::min<uint32_t>(chunkPaths, segn[sg] - done);
                const unsigned long long e = lists[(size_t)sg * R().poolChunks + j];
                const uint32_t c = j == 0 ? 1u + (uint32_t)sg : (uint32_t)e;
                if (c == 0 || c >= (uint32_t)R().poolChunks || (j != 0 && (uint32_t)(e >> 32) != gen))
                    return fail(PT_ERR_DEVICE, "pt_debug_trace_paths: corrupt chunk list");
                const size_t first = (size_t)c << R().prm.chunkShift;
                HIPCHECK(hipMemcpy(bufA.data(), pb.arrA(first), (size_t)m * 16, hipMemcpyDeviceToHost));
                HIPCHECK(hipMemcpy(bufB.data(), pb.arrB(first), (size_t)m * 16, hipMemcpyDeviceToHost));
                if (hb == 0) HIPCHECK(hipMemcpy(bufC.data(), pb.arrC(first), (size_t)m * 12, hipMemcpyDeviceToHost));
                for (uint32_t i = 0; i < m; ++i) {
                    const float *a = &bufA[4 * (size_t)i], *b = &bufB[4 * (size_t)i], *cc = &bufC[3 * (size_t)i];
                    if (hb != 0) {
                        uint32_t h;
                        memcpy(&h, &b[2], sizeof h);
                        float col[3] = {1.0f, 1.0f, 1.0f};
                        for (int s = 0; s < bounces; ++s, h >>= hb) {
                            const uint32_t code = h & ((1u << hb) - 1u);
                            if ((code >> 1) >= (uint32_t)hmat.size()) return fail(PT_ERR_DEVICE, "pt_debug_trace_paths: corrupt history word");
                            const float *t = (code & 1u) ? hmat[code >> 1].specColor : hmat[code >> 1].color;
                            for (int q = 0; q < 3; ++q) col[q] = col[q] * t[q];
                        }
                        const float v[kNumArrays] = {a[0], a[1], a[2], a[3], b[0], b[1], col[0], col[1], col[2], 0.0f, b[3]};      // (no hash in such a pool; nobody reads that column)
                        for (int k = 0; k < kNumArrays; ++k) cols[k][off + i] = v[k];
                        continue;
                    }
                    const float v[kNumArrays] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], cc[0], cc[1], cc[2]};
                    for (int k = 0; k < kNumArrays; ++k) cols[k][off + i] = v[k];
                }
                off += m;
            }
    }
    // (array C's third word: pixelIndex | batch index << pixBits; this private run traces ONE iteration: the batch index is 0)
    const int *pixcol = reinterpret_cast<const int *>(cols[10].data());
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return pixcol[x] < pixcol[y]; });
    float *dst[3] = {origin3, dir3, color3};
    for (size_t i = 0; i < n; ++i) {
        const size_t src = order[i];
        for (int grp = 0; grp < 3; ++grp)
            if (dst[grp])
                for (int c = 0; c < 3; ++c) dst[grp][3 * i + c] = cols[grp * 3 + c][src];
        if (pixelIndex) pixelIndex[i] = pixcol[src];
    }
    return PT_OK;
}

// ---- primitive tests over host arrays ------------------------------------------------------------------
int pt_test_force_fault(int which) {
    if (count_devices() < 1) return fail(PT_ERR_NO_GPU, "no HIP device");
    if (which != 0 && which != 2) return fail(PT_ERR_INVALID, "pt_test_force_fault: which must be 0 (clear) or 2 (the renderer's fault word)");
    if (!R().init) return fail(PT_ERR_NOT_INIT, "pt_test_force_fault before pt_init");
    HIPCHECK(hipDeviceSynchronize());
    const uint32_t word = which == 2 ? 1u : 0u;
    for (int i = 0; i < (which == 2 ? 1 : R().nslots); ++i) HIPCHECK(hipMemcpy(&R().slot[i].ctrl.p->error, &word, sizeof word, hipMemcpyHostToDevice));
    if (R().hostFault) *R().hostFault = word;
    return PT_OK;
}

// (host only) the form of k_bounce the renderer's selector picks for a state: bit 0 first, 1 dof, 2 many, 3 sweptCubes, 4 mesh, 5 grouped, 6 tex,
// 7 bump, 8 plain -> the nine template flags, bit 0 FIRST .. bit 8 BUMP; an error when that form is not instantiated
int pt_test_bounce_form(uint32_t state_bits, uint32_t *form_bits) {
    if (!form_bits || state_bits >= 512u) return fail(PT_ERR_INVALID, "pt_test_bounce_form: bad argument");
    const auto bit = [state_bits](int i) { return ((state_bits >> i) & 1u) != 0; };
    const uint32_t f = bounce_form(bit(0), bit(1), bit(2), bit(3), bit(4), bit(5), bit(6), bit(7), bit(8));
    if (!bounce_kernel(f)) return fail(PT_ERR_INVALID, "pt_test_bounce_form: no k_bounce form 0x%x", f);
    *form_bits = f;
    return PT_OK;
}

// a plan's state in pt_test_bounce_form's bit order with `first` (bit 0) clear
uint32_t plan_state_bits(const PlanScalars &p) {
    const bool s[9] = {false, p.dof, p.many, p.sweptCubes, p.mesh, p.grouped, p.tex, p.bump, p.plain};
    uint32_t bits = 0u;
    for (int i = 0; i < 9; ++i) bits |= (s[i] ? 1u : 0u) << i;
    return bits;
}

// (host only) the state pt_init left in this library's renderer: the plan it stored
int pt_test_renderer_state(uint32_t *state_bits) {
    if (!state_bits) return fail(PT_ERR_INVALID, "pt_test_renderer_state: bad argument");
    if (!R().init) return fail(PT_ERR_NOT_INIT, "pt_test_renderer_state before pt_init");
    *state_bits = plan_state_bits(R());
    return PT_OK;
}

// (host only) what pt_init would plan for the scene -- its arguments, and the meshes, textures and bindings registered with this library --
// or its refusal: plan_scene, no device
int pt_test_scene_plan(const PtCamera *cam, const PtGeom *geoms, int ngeoms, const PtMaterial *mats, int nmats, int traceDepth, const PtOptions *opts,
                       PtTestPlanSummary *out) {
    if (!out) return fail(PT_ERR_INVALID, "pt_test_scene_plan: bad argument");
    ScenePlan p;
    PTCHECK(plan_scene(SceneIn(cam, geoms, ngeoms, mats, nmats, traceDepth, effective_options(opts), R().reg), p));
    *out = PtTestPlanSummary{plan_state_bits(p), p.prm.nBinned, p.prm.nWalls, p.prm.nSphCull, p.prm.nSphGroups, p.prm.nLocalPad, p.prm.firstSkipped, p.poolChunks,
                             (uint64_t)p.ldsBytes, (uint64_t)p.ldsBytesNext, p.prm.histBits, p.prm.grpLds};
    return PT_OK;
}

// (host only) the swept primitives' table as pt_init would build it for the scene: the plan's own phases up to plan_swept (which calls
// build_sphere_clusters and build_sphere_groups), so a scene that plan_lds refuses afterwards still shows its table
int pt_test_sphere_groups(const PtCamera *cam, const PtGeom *geoms, int ngeoms, const PtMaterial *mats, int nmats, int traceDepth, const PtOptions *opts,
                          int32_t *table, float *entries5, int32_t table_cap, float *balls4, int32_t balls_cap, int32_t info6[6], float bounds2[2]) {
    if (!table || !entries5 || !balls4 || !info6 || !bounds2 || table_cap < 0 || balls_cap < 0) return fail(PT_ERR_INVALID, "pt_test_sphere_groups: bad argument");
    ScenePlan p;
    const SceneIn in(cam, geoms, ngeoms, mats, nmats, traceDepth, effective_options(opts), R().reg);
    PTCHECK(check_scene(in));
    PTCHECK(plan_frame(in, p));
    PTCHECK(plan_emitters(in, p));
    PTCHECK(plan_pools(in, p));
    PTCHECK(plan_geoms(in, p));
    PTCHECK(plan_camera_cull(in, p));
    plan_bins(in, p);
    plan_walls(in, p);
    PTCHECK(plan_textures(in, p));
    PTCHECK(plan_bump_maps(in, p));
    PTCHECK(plan_swept(in, p));
    const KParams &k = p.prm;
    if ((int)p.sc.size() > table_cap) return fail(PT_ERR_INVALID, "pt_test_sphere_groups: table_cap too small (%d entries)", (int)p.sc.size());
    if (k.nSphGroups > balls_cap) return fail(PT_ERR_INVALID, "pt_test_sphere_groups: balls_cap too small (%d groups)", k.nSphGroups);
    for (size_t i = 0; i < p.sc.size(); ++i) {
        const SphereCull &e = p.sc[i];
        table[i] = e.geom;
        const float v[5] = {e.centre[0], e.centre[1], e.centre[2], e.cullR2, e.cullK};
        memcpy(entries5 + 5 * i, v, sizeof v);
    }
    for (int g = 0; g < k.nSphGroups; ++g) {
        const SphereCull &e = p.groups[(size_t)g];
        const float v[4] = {e.centre[0], e.centre[1], e.centre[2], e.cullR2};
        memcpy(balls4 + 4 * g, v, sizeof v);
    }
    const int32_t info[6] = {(int32_t)p.sc.size(), k.sphN0, k.grpN0, k.nSphGroups, p.many ? p.nswept : 0, p.grouped ? 1 : 0};
    memcpy(info6, info, sizeof info);
    bounds2[0] = k.grpOMax;
    bounds2[1] = k.sphDirScale;
    return PT_OK;
}

int64_t pt_test_live_device_buffers(void) { return (int64_t)g_liveDevBufs.load(); }
int64_t pt_test_live_handles(void) { return (int64_t)g_liveHandles.load(); }

int pt_test_pose_tables(int64_t out[6]) {
    if (!R().init) return fail(PT_ERR_NOT_INIT, "pt_test_pose_tables before pt_init");
    if (!out) return fail(PT_ERR_INVALID, "pt_test_pose_tables: null");
    const auto &t = R().tables;
    out[0] = R().poses.empty() ? 1 : (int64_t)R().poses.size();
    out[1] = t.ownBuffers; out[2] = t.ownBytes; out[3] = t.sharedBuffers; out[4] = t.sharedBytes; out[5] = t.allOwnBytes;
    return PT_OK;
}

int pt_test_group_fail_next_reduce(PtGroup *g, int count) {
    if (!g || count < 0) return fail(PT_ERR_INVALID, "pt_test_group_fail_next_reduce: bad argument");
    g->failReduces = count;
    return PT_OK;
}

// A group on VIRTUAL devices: pt_group_create's second half (pt_group.h: group_build) over a map that groups the members by vdev[i] instead of
// by HIP ordinal, with the emulated reduce's table -- or the host gather -- as its collective.
int pt_test_group_create_virtual(PtGroup **out, int n, const int32_t *vdev, int collective) {
    if (!out || !vdev || n < 1 || n > 64) return fail(PT_ERR_INVALID, "pt_test_group_create_virtual: 1..64 members");
    if (collective != 0 && collective != 1) return fail(PT_ERR_INVALID, "pt_test_group_create_virtual: collective 0 (host gather) or 1 (emulated reduce)");
    if (count_devices() < 1) return fail(PT_ERR_NO_GPU, "pt_test_group_create_virtual: no HIP device");
    if (vdev[0] != 0) return fail(PT_ERR_INVALID, "pt_test_group_create_virtual: member 0 sits on virtual device 0, the root");
    for (int i = 0; i < n; ++i)
        if (vdev[i] < 0 || vdev[i] >= kEmuMaxRanks) return fail(PT_ERR_INVALID, "pt_test_group_create_virtual: virtual device %d of %d", vdev[i], kEmuMaxRanks);
    int hip = 0;
    HIPCHECK(hipGetDevice(&hip));
    PtGroup *g = new (std::nothrow) PtGroup();
    if (!g) return fail(PT_ERR_INVALID, "pt_test_group_create_virtual: out of memory");
    for (int i = 0; i < n; ++i) group_place(g, vdev[i], hip);
    return group_build(out, g, EmulatedReduce::table(), collective, "pt_test_group_create_virtual");
}

// The emulated reduce alone, through its function table as a group calls it: `ranks` send buffers of `count` floats uploaded to the device, one
// stream per rank, GroupStart, one Reduce per rank (root 0; in_place: the root receives into its own send buffer), GroupEnd; then the streams
// are waited for and the root's receive buffer and every rank's send buffer are read back.
int pt_test_emulated_reduce(const float *const *send_host, int ranks, int64_t count, int in_place, float *recv_host, float *const *send_after_host) {
    if (!send_host || !recv_host || ranks < 1 || ranks > kEmuMaxRanks || count < 1) return fail(PT_ERR_INVALID, "pt_test_emulated_reduce: bad argument");
    if (count_devices() < 1) return fail(PT_ERR_NO_GPU, "no HIP device");
    const Rccl &api = *EmulatedReduce::table();
    struct Rank {
        DevBuf<float> send;
        Stream stream;
        void *comm = nullptr;
    };
    std::vector<Rank> rk(ranks);
    DevBuf<float> recv;
    std::vector<void *> comms(ranks, nullptr);
    int rc = PT_OK, r = 0;
    for (int i = 0; i < ranks && rc == PT_OK; ++i) {
        rc = rk[i].send.upload(send_host[i], (size_t)count);
        if (rc == PT_OK && rk[i].stream.create(hipStreamNonBlocking) != PT_OK) rc = fail(PT_ERR_HIP, "pt_test_emulated_reduce: no stream");
    }
    if (rc == PT_OK && !in_place) rc = recv.alloc_zeroed((size_t)count);
    if (rc == PT_OK && (r = api.CommInitAll(comms.data(), ranks, nullptr)) != 0) rc = fail(PT_ERR_HIP, "pt_test_emulated_reduce: CommInitAll: %s", api.GetErrorString(r));
    if (rc == PT_OK) {
        for (int i = 0; i < ranks; ++i) rk[i].comm = comms[i];
        if (hipDeviceSynchronize() != hipSuccess) rc = fail(PT_ERR_HIP, "pt_test_emulated_reduce: the uploads failed");      // (the uploads: the streams below are non-blocking)
    }
    if (rc == PT_OK) {
        r = api.GroupStart();
        if (r == 0) {
            for (int i = 0; i < ranks; ++i) {
                float *const dst = i != 0 ? nullptr : in_place ? rk[0].send.p : recv.p;
                const int ri = api.Reduce(rk[i].send.p, dst, (size_t)count, kNcclFloat, kNcclSum, 0, rk[i].comm, rk[i].stream);
                if (ri != 0 && r == 0) r = ri;
            }
            const int r2 = api.GroupEnd();
            if (r == 0) r = r2;
        }
        if (r != 0) rc = fail(PT_ERR_HIP, "pt_test_emulated_reduce: %s", api.GetErrorString(r));
    }
    // every rank's stream: the operation is complete on each of them
    for (int i = 0; i < ranks; ++i)
        if (rk[i].stream && hipStreamSynchronize(rk[i].stream) != hipSuccess && rc == PT_OK) rc = fail(PT_ERR_HIP, "pt_test_emulated_reduce: a rank's stream failed");
    if (rc == PT_OK && hipMemcpy(recv_host, in_place ? rk[0].send.p : recv.p, (size_t)count * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(PT_ERR_HIP, "pt_test_emulated_reduce: read-back");
    for (int i = 0; i < ranks && rc == PT_OK && send_after_host; ++i)
        if (send_after_host[i] && hipMemcpy(send_after_host[i], rk[i].send.p, (size_t)count * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(PT_ERR_HIP, "pt_test_emulated_reduce: read-back");
    for (int i = 0; i < ranks; ++i)      // (the communicators before the streams, which go with `rk`)
        if (rk[i].comm) (void)api.CommDestroy(rk[i].comm);
    return rc;
}

// ---- what the entry points below share: launch, counters, grids, packed scenes ------------------------------
#define NEED_GPU() do { if (count_devices() < 1) return fail(PT_ERR_NO_GPU, "no HIP device"); } while (0)

extern "C++" {     // (templates among them: pt_api.hip includes this file inside its extern "C" block)

constexpr int kTestThreads = 256;     // every test kernel runs in one-dimensional blocks of this size
inline dim3 blocks_for(long long n) { return dim3((unsigned)((n + kTestThreads - 1) / kTestThreads)); }      // one lane per element

// a sweep's grid: `rays` at `per_thread` per lane, at least one block, at most `cap` (a lane's stream is a function of its global index:
// the sweeps' counts depend on this)
inline dim3 sweep_grid(long long rays, int per_thread, int threads, long long cap) {
    const long long perBlock = (long long)per_thread * threads;
    return dim3((unsigned)std::min(std::max((rays + perBlock - 1) / perBlock, 1ll), cap));
}

// every launch of a test kernel: on the null stream, checked, waited for
template <typename... P, typename... A>
int launch_wait(void (*kernel)(P...), dim3 grid, size_t ldsBytes, const A &...args) {
    hipLaunchKernelGGL(kernel, grid, dim3(kTestThreads), ldsBytes, nullptr, args...);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    return PT_OK;
}

// launch() on the null stream, once; with `ms`: once untimed, then `reps` times between two events, ms[r] the r-th one's time
template <class Launch>
int timed_launches(int reps, float *ms, Launch launch) {
    Event ev[2];
    if (ms) for (Event &e : ev) PTCHECK(e.create(hipEventDefault));
    for (int r = 0; r < (ms ? reps + 1 : 1); ++r) {
        if (ms && r) HIPCHECK(hipEventRecord(ev[0], nullptr));
        PTCHECK(launch());
        if (ms && r) {
            HIPCHECK(hipEventRecord(ev[1], nullptr));
            HIPCHECK(hipEventSynchronize(ev[1]));
            HIPCHECK(hipEventElapsedTime(&ms[r - 1], ev[0], ev[1]));
        }
    }
    return PT_OK;
}

template <typename T>
int download(T *host, const DevBuf<T> &buf, size_t n) {
    HIPCHECK(hipMemcpy(host, buf.p, n * sizeof(T), hipMemcpyDeviceToHost));
    return PT_OK;
}

// the N 64-bit counters of a sweep: zeroed on the device, read into h after the launch and handed out in order
template <int N>
struct Counters {
    DevBuf<unsigned long long> d;
    unsigned long long h[N] = {};
    int zero() { return d.alloc_zeroed(N); }
    unsigned long long *at(int i) const { return d.p + i; }
    int read(std::initializer_list<uint64_t *> outs = {}) {
        PTCHECK(download(h, d, N));
        int i = 0;
        for (uint64_t *o : outs) *o = h[i++];
        return PT_OK;
    }
};

// the primitives as pt_init packs them (`eye`: with the object-space eye of the camera-ray tests), or the refusal of a type outside `allowed`
enum : unsigned { kSpheres = 1u << PT_SPHERE, kCubes = 1u << PT_CUBE, kAnyGeom = ~0u };
int pack_geoms(const PtGeom *geoms, int ngeoms, unsigned allowed, const float *eye, const char *fn, std::vector<GeomDev> &hg) {
    hg.resize(ngeoms);
    for (int i = 0; i < ngeoms; ++i) {
        const int t = geoms[i].type;
        if (allowed != kAnyGeom && (t < 0 || t > 31 || !((allowed >> t) & 1u)))
            return fail(PT_ERR_INVALID, "%s: %s only", fn, allowed == kCubes ? "cubes" : "spheres and cubes");
        pack_geom(geoms[i], hg[i], eye);
    }
    return PT_OK;
}

// the bounding box of every bounded primitive: where the cluster and group sweeps start their rays "from the scene"
void scene_extent(const std::vector<GeomDev> &hg, F3 &slo, F3 &shi) {
    slo = F3{INFINITY, INFINITY, INFINITY};
    shi = F3{-INFINITY, -INFINITY, -INFINITY};
    for (const GeomDev &g : hg) {
        const float r = g.boundR;
        if (!std::isfinite(r)) continue;
        slo = F3{std::min(slo.x, g.centre[0] - r), std::min(slo.y, g.centre[1] - r), std::min(slo.z, g.centre[2] - r)};
        shi = F3{std::max(shi.x, g.centre[0] + r), std::max(shi.y, g.centre[1] + r), std::max(shi.z, g.centre[2] + r)};
    }
}

// the rays of an intersect test and what its kernel keeps per ray: t, the hit point and normal (in: the caller's sentinels), outside, culled
struct RayHits {
    DevBuf<float> rays, t, p, n;
    DevBuf<int> outside, culled;
    int up(const float *rays6, int count, const float *p3, const float *n3, const int32_t *out) {
        PTCHECK(rays.upload(rays6, (size_t)count * 6));
        PTCHECK(p.upload(p3, (size_t)count * 3));
        PTCHECK(n.upload(n3, (size_t)count * 3));
        PTCHECK(outside.upload(out, count));
        PTCHECK(t.alloc(count));
        return culled.alloc(count);
    }
    int down(int count, float *ht, float *p3, float *n3, int32_t *out, int32_t *cull) {
        PTCHECK(download(ht, t, count));
        PTCHECK(download(p3, p, (size_t)count * 3));
        PTCHECK(download(n3, n, (size_t)count * 3));
        PTCHECK(download(out, outside, count));
        return cull ? download(cull, culled, count) : PT_OK;
    }
};

// One mesh as pt_init lays it out: the records, and (upload) the packed geom with its root and stride, the walk's stacks in LDS -- or the
// refusal of a hierarchy too deep for them -- and the device copies
struct MeshFixture {
    std::vector<ptd::MeshUnit> recs;
    float box[6];
    ptm::MeshLayout lay;
    GeomDev hg;
    size_t stackBytes = 0;
    DevBuf<GeomDev> dg;
    DevBuf<ptd::MeshUnit> drec;
    void append(const float *tris, int ntris, bool flat, const float *normals = nullptr, const int32_t *mats = nullptr) {
        lay = ptm::appendMesh(tris, ntris, flat, recs, box, normals, mats);
    }
    int upload(const PtGeom &geom, const char *fn) {
        pack_geom(geom, hg, nullptr, box);
        hg.meshRoot = lay.root;
        hg.meshStride = lay.stride;
        stackBytes = (size_t)std::max(lay.stackNeed, 1) * kTestThreads * sizeof(uint32_t);
        if (stackBytes > 64 * 1024) return fail(PT_ERR_INVALID, "%s: the hierarchy needs %d stack levels", fn, lay.stackNeed);
        PTCHECK(dg.upload(&hg, 1));
        return drec.upload(recs);
    }
    const float4 *units() const { return reinterpret_cast<const float4 *>(drec.p); }
};

// One (camera, primitive set) as pt_init derives it.  pack: the camera constants with the row divisor, the packed primitives (object-space
// eye).  cull: pack, then the rectangles, their union and the per-row lists.  list: a shard's packed work list without a length cap.
struct CameraFixture {
    KParams k;
    std::vector<GeomDev> hg;
    CameraCull cc;
    int pack(const PtCamera *cam, const PtGeom *geoms, int ngeoms, unsigned allowed, long long maxPixels, const char *fn) {
        if (cam->resolution[0] < 1 || cam->resolution[1] < 1 || (long long)cam->resolution[0] * cam->resolution[1] > maxPixels)
            return fail(PT_ERR_INVALID, "%s: bad resolution", fn);
        memset(&k, 0, sizeof k);
        camera_params(*cam, k);
        k.ngeoms = ngeoms;
        magic_divisor((uint32_t)k.W, k.magicW, k.shiftW);
        return pack_geoms(geoms, ngeoms, allowed, k.pos, fn, hg);
    }
    int cull(const PtCamera *cam, const PtGeom *geoms, int ngeoms, unsigned allowed, long long maxPixels, const char *fn) {
        PTCHECK(pack(cam, geoms, ngeoms, allowed, maxPixels, fn));
        build_camera_cull(geoms, ngeoms, k, false, std::vector<const float *>(ngeoms, nullptr), hg, cc);
        for (int a = 0; a < 4; ++a) k.sceneRect[a] = cc.sceneRect[a];
        return PT_OK;
    }
    // (`resolve`: as for the untextured forms -- one-cube signatures split by the face their pixels are resolved to, camera_face_certificate --
    // with the per-wave faces beside it; `built`: false where pt_init would build no list)
    int list(const PtGeom *geoms, int shard_rank, int shard_count, bool resolve, const char *fn, CameraList &cl, bool &built) const {
        if (shard_count < 1 || shard_rank < 0 || shard_rank >= shard_count) return fail(PT_ERR_INVALID, "%s: bad shard", fn);
        CameraResolve cr;
        if (resolve) build_camera_resolve(geoms, k.ngeoms, k, hg, cr);
        built = build_camera_list(cc, k.W, k.H, shard_rank, shard_count, std::numeric_limits<long long>::max(), cl, resolve ? &cr : nullptr);
        return PT_OK;
    }
};
constexpr long long kAnyResolution = std::numeric_limits<long long>::max();

}  // extern "C++"

int pt_test_utilhash(const uint32_t *in, uint32_t *out, int n) {
    NEED_GPU();
    if (n <= 0) return PT_OK;
    DevBuf<uint32_t> a, b;
    PTCHECK(a.upload(in, n));
    PTCHECK(b.alloc(n));
    PTCHECK(launch_wait(k_test_utilhash, blocks_for(n), 0, a.p, b.p, n));
    return download(out, b, n);
}

int pt_test_rng(const uint32_t *seeds, int nseeds, int ndraws, float *u01_out) {
    NEED_GPU();
    if (nseeds <= 0 || ndraws <= 0) return PT_OK;
    DevBuf<uint32_t> a;
    DevBuf<float> b;
    PTCHECK(a.upload(seeds, nseeds));
    PTCHECK(b.alloc((size_t)nseeds * ndraws));
    PTCHECK(launch_wait(k_test_rng, blocks_for(nseeds), 0, a.p, nseeds, ndraws, b.p));
    return download(u01_out, b, (size_t)nseeds * ndraws);
}

int pt_test_intersect(const PtGeom *geoms, int ngeoms, const int32_t *geom_index, const float *rays, int n, float *t,
                      float *p3, float *n3, int32_t *outside) {
    NEED_GPU();
    if (n <= 0) return PT_OK;
    for (int i = 0; i < n; ++i)
        if (geom_index[i] < 0 || geom_index[i] >= ngeoms) return fail(PT_ERR_INVALID, "pt_test_intersect: geom index out of range");
    std::vector<GeomDev> hg;
    PTCHECK(pack_geoms(geoms, ngeoms, kAnyGeom, nullptr, "pt_test_intersect", hg));
    DevBuf<GeomDev> dg;
    DevBuf<int> di;
    RayHits r;
    PTCHECK(dg.upload(hg));
    PTCHECK(di.upload(geom_index, n));
    PTCHECK(r.up(rays, n, p3, n3, outside));
    PTCHECK(launch_wait(k_test_intersect, blocks_for(n), 0, dg.p, di.p, r.rays.p, n, r.t.p, r.p.p, r.n.p, r.outside.p));
    return r.down(n, t, p3, n3, outside, nullptr);
}

int pt_test_mesh_intersect(const PtGeom *geom, const float *tris, int ntris, int flat, const float *rays, int n, float *t,
                           float *p3, float *n3, int32_t *outside, int32_t *culled) {
    NEED_GPU();
    if (!geom || !tris || ntris < 1 || geom->type != PT_MESH) return fail(PT_ERR_INVALID, "pt_test_mesh_intersect: bad argument");
    if (n <= 0) return PT_OK;
    MeshFixture m;
    RayHits r;
    m.append(tris, ntris, flat != 0);
    PTCHECK(m.upload(*geom, "pt_test_mesh_intersect"));
    PTCHECK(r.up(rays, n, p3, n3, outside));
    PTCHECK(launch_wait(k_test_mesh, blocks_for(n), m.stackBytes, m.dg.p, m.units(), r.rays.p, n, r.t.p, r.p.p, r.n.p, r.outside.p, r.culled.p));
    return r.down(n, t, p3, n3, outside, culled);
}

int pt_test_mesh_intersect2(const PtGeom *geom, const float *tris, const float *normals, const int32_t *mats, int ntris, int flat,
                            const float *rays, int n, float *t, float *p3, float *n3, int32_t *outside, int32_t *culled, int32_t *tri,
                            int32_t *face_mat) {
    NEED_GPU();
    if (!geom || !tris || ntris < 1 || geom->type != PT_MESH || !tri || !face_mat) return fail(PT_ERR_INVALID, "pt_test_mesh_intersect2: bad argument");
    if (n <= 0) return PT_OK;
    // the records twice: as pt_init lays them out, and with 1 + the triangle's file index in the material's word (same geometry, same refs)
    MeshFixture m, tagged;
    std::vector<int> index((size_t)ntris);
    for (int i = 0; i < ntris; ++i) index[(size_t)i] = i;
    m.append(tris, ntris, flat != 0, normals, mats);
    tagged.append(tris, ntris, flat != 0, normals, index.data());
    if (tagged.lay.root != m.lay.root || tagged.lay.stride != m.lay.stride || tagged.lay.stackNeed != m.lay.stackNeed || tagged.recs.size() != m.recs.size())
        return fail(PT_ERR_INVALID, "pt_test_mesh_intersect2: the two record arrays differ in layout");
    RayHits r;
    DevBuf<int> dtri, dfm;
    PTCHECK(m.upload(*geom, "pt_test_mesh_intersect2"));
    PTCHECK(tagged.drec.upload(tagged.recs));
    PTCHECK(r.up(rays, n, p3, n3, outside));
    PTCHECK(dtri.alloc(n));
    PTCHECK(dfm.alloc(n));
    PTCHECK(launch_wait(k_test_mesh2, blocks_for(n), m.stackBytes, m.dg.p, m.units(), tagged.units(), r.rays.p, n, r.t.p, r.p.p, r.n.p, r.outside.p,
                        r.culled.p, dtri.p, dfm.p));
    PTCHECK(r.down(n, t, p3, n3, outside, culled));
    PTCHECK(download(tri, dtri, n));
    return download(face_mat, dfm, n);
}

int pt_test_mesh_cull_sweep(const PtGeom *geom, const float *tris, int ntris, uint64_t seed, int64_t rays, uint64_t *culled,
                            uint64_t *violations, uint64_t *hits) {
    NEED_GPU();
    if (!geom || !tris || ntris < 1 || geom->type != PT_MESH || !culled || !violations || !hits || rays < 0)
        return fail(PT_ERR_INVALID, "pt_test_mesh_cull_sweep: bad argument");
    MeshFixture m;
    Counters<3> cnt;
    m.append(tris, ntris, false);
    PTCHECK(m.upload(*geom, "pt_test_mesh_cull_sweep"));
    if (!std::isfinite(m.hg.cullR2)) return fail(PT_ERR_INVALID, "pt_test_mesh_cull_sweep: this mesh is never culled");
    PTCHECK(cnt.zero());
    const int per_thread = 64;
    PTCHECK(launch_wait(k_sweep_mesh_cull, sweep_grid(rays, per_thread, kTestThreads, 1 << 20), m.stackBytes, m.dg.p, m.units(), seed, per_thread,
                        cnt.at(0), cnt.at(1), cnt.at(2)));
    return cnt.read({culled, violations, hits});
}

// host only: no GPU is touched
int pt_test_mesh_bvh(const float *tris, int ntris, int octant, uint32_t *units4, int *nrecs, int *stack_need) {
    if (!tris || ntris < 1 || !units4 || !nrecs || !stack_need || octant < 0 || octant > 7) return fail(PT_ERR_INVALID, "pt_test_mesh_bvh: bad argument");
    MeshFixture m;
    m.append(tris, ntris, false);
    const std::vector<ptd::MeshUnit> &recs = m.recs;
    const ptm::MeshLayout lay = m.lay;
    // units of 16 bytes: the triangles (three each), [one unit of padding when their count is odd,] this octant's inner nodes (two each)
    const uint32_t triUnits = (uint32_t)ptd::kMeshTriUnits * (uint32_t)ntris, pad = triUnits % 2u;
    const uint32_t total = triUnits + pad + lay.stride;
    if ((int)total > *nrecs) return fail(PT_ERR_INVALID, "pt_test_mesh_bvh: %u units do not fit %d", total, *nrecs);
    // refs rebased to this array: triangle i -> kMeshLeaf | 3 i, inner node j of the copy -> triUnits + pad + 2 j
    const uint32_t innerBase = triUnits + pad + (uint32_t)octant * lay.stride;
    auto rebase = [&](uint32_t r) { return (r & ptd::kMeshLeaf) ? r : r - innerBase + triUnits + pad; };
    memcpy(units4, recs.data(), (size_t)(triUnits + pad) * sizeof(ptd::MeshUnit));
    for (uint32_t j = 0; j < lay.stride; ++j) {
        ptd::MeshUnit n = recs[(size_t)innerBase + j];
        n.w[3] = rebase(n.w[3]);
        memcpy(units4 + 4 * ((size_t)triUnits + pad + j), &n, sizeof n);
    }
    *nrecs = (int)total;
    *stack_need = lay.stackNeed;
    return PT_OK;
}

// the walls exactly as pt_init chooses and numbers them among `geoms`, cubes all (no primitive of the set is binned here)
static int test_choose_walls(const PtGeom *geoms, int ngeoms, const char *fn, std::vector<GeomDev> &hg, KParams &k, std::vector<WallBox> &hw,
                             std::vector<int> &wallGeom) {
    PTCHECK(pack_geoms(geoms, ngeoms, kCubes, nullptr, fn, hg));
    memset(&k, 0, sizeof k);
    hw.resize(kWallMax);
    choose_walls(geoms, ngeoms, hg, k, hw, wallGeom);
    return PT_OK;
}

// host only: no GPU is touched
int pt_test_wall_planes(const PtGeom *geoms, int ngeoms, float *planes, int32_t *wall_geom, int32_t *nslot, int32_t *nplane, int32_t *nwalls) {
    if (!geoms || ngeoms < 1 || !planes || !wall_geom || !nslot || !nplane || !nwalls) return fail(PT_ERR_INVALID, "pt_test_wall_planes: bad argument");
    std::vector<GeomDev> hg;
    KParams k;
    std::vector<WallBox> hw;
    std::vector<int> wallGeom;
    PTCHECK(test_choose_walls(geoms, ngeoms, "pt_test_wall_planes", hg, k, hw, wallGeom));
    *nslot = k.nSlotWalls; *nplane = k.nPlaneWalls; *nwalls = k.nWalls;
    for (int w = 0; w < kWallMax; ++w) {
        for (int q = 0; q < 5; ++q) planes[5 * w + q] = w < k.nPlaneWalls ? k.planeN[w][q] : 0.0f;
        wall_geom[w] = w < (int)wallGeom.size() ? wallGeom[w] : -1;
    }
    return PT_OK;
}

int pt_test_sphere_cull_sweep(const PtGeom *geoms, int ngeoms, uint64_t seed, int64_t rays, uint64_t *culled,
                              uint64_t *violations) {
    NEED_GPU();
    if (!geoms || ngeoms < 1 || !culled || !violations || rays < 0) return fail(PT_ERR_INVALID, "pt_test_sphere_cull_sweep: bad argument");
    std::vector<GeomDev> hg;
    PTCHECK(pack_geoms(geoms, ngeoms, kAnyGeom, nullptr, "pt_test_sphere_cull_sweep", hg));
    DevBuf<GeomDev> dg;
    Counters<2> cnt;
    PTCHECK(dg.upload(hg));
    PTCHECK(cnt.zero());
    const int per_thread = 256;
    PTCHECK(launch_wait(k_sweep_sphere_cull, sweep_grid(rays, per_thread, kTestThreads, 1 << 20), 0, dg.p, ngeoms, seed, per_thread, cnt.at(0), cnt.at(1)));
    return cnt.read({culled, violations});
}

int pt_test_sphere_halfline_sweep(const PtGeom *geoms, int ngeoms, uint64_t seed, int64_t rays, uint64_t *culled, uint64_t *behind,
                                  uint64_t *violations) {
    NEED_GPU();
    if (!geoms || ngeoms < 1 || !culled || !behind || !violations || rays < 0) return fail(PT_ERR_INVALID, "pt_test_sphere_halfline_sweep: bad argument");
    std::vector<GeomDev> hg;
    PTCHECK(pack_geoms(geoms, ngeoms, kSpheres | kCubes, nullptr, "pt_test_sphere_halfline_sweep", hg));
    DevBuf<GeomDev> dg;
    Counters<3> cnt;
    PTCHECK(dg.upload(hg));
    PTCHECK(cnt.zero());
    const int per_thread = 256;
    PTCHECK(launch_wait(k_sweep_sphere_halfline, sweep_grid(rays, per_thread, kTestThreads, 1 << 20), 0, dg.p, ngeoms, seed, per_thread, cnt.at(0),
                        cnt.at(1), cnt.at(2)));
    return cnt.read({culled, behind, violations});
}

// the sweeps' table: the primitives of a scene of spheres and cubes, packed, and every sphere with its culling data as pt_init packs it
// (thresholds scaled for the folded K |oc|^2 term)
static int pack_sphere_cull(const PtGeom *geoms, int ngeoms, const char *fn, std::vector<GeomDev> &hg, std::vector<SphereCull> &sc) {
    PTCHECK(pack_geoms(geoms, ngeoms, kSpheres | kCubes, nullptr, fn, hg));
    sc.clear();
    for (int i = 0; i < ngeoms; ++i) {
        if (geoms[i].type != PT_SPHERE) continue;
        SphereCull e;
        memset(&e, 0, sizeof e);
        for (int a = 0; a < 3; ++a) e.centre[a] = hg[i].centre[a];
        e.cullR2 = hg[i].cullR2;
        e.cullK = hg[i].cullK + kUnitDirSlack;
        e.geom = i;
        sc.push_back(e);
    }
    double kmax = 0.0;
    for (const SphereCull &e : sc) kmax = std::max(kmax, (double)e.cullK);
    const float sdir = std::nextafter((float)std::sqrt(1.0 / (1.0 - kmax)), INFINITY);
    for (SphereCull &e : sc)
        if (std::isfinite(e.cullR2)) e.cullR2 = std::nextafter((float)((double)e.cullR2 * (double)sdir * (double)sdir), INFINITY);
    return PT_OK;
}

// the two clusters exactly as pt_init builds them for this scene (no primitive binned: binning only moves the choice of the split)
struct SphereClusters {
    std::vector<GeomDev> hg;
    std::vector<SphereCull> sc;
    int n0 = 0;
    float omax = 0.0f, box[2][8];
    int build(const PtGeom *geoms, int ngeoms, const char *fn) {
        PTCHECK(pack_sphere_cull(geoms, ngeoms, fn, hg, sc));
        if (!build_sphere_clusters(geoms, ngeoms, hg, std::vector<int>(), sc, n0, omax, box)) return fail(PT_ERR_INVALID, "%s: no clusters for this scene", fn);
        return PT_OK;
    }
    void info(float *info18) const {
        info18[0] = omax; info18[1] = (float)n0;
        for (int g = 0; g < 2; ++g) for (int q = 0; q < 8; ++q) info18[2 + 8 * g + q] = box[g][q];
    }
};

int pt_test_sphere_clusters(const PtGeom *geoms, int ngeoms, float *info18, int32_t *table, int32_t table_cap, int32_t *ntable) {
    if (!geoms || ngeoms < 2 || !info18 || !table || !ntable) return fail(PT_ERR_INVALID, "pt_test_sphere_clusters: bad argument");
    SphereClusters c;
    PTCHECK(c.build(geoms, ngeoms, "pt_test_sphere_clusters"));
    if ((int)c.sc.size() > table_cap) return fail(PT_ERR_INVALID, "pt_test_sphere_clusters: table_cap too small (%d entries)", (int)c.sc.size());
    c.info(info18);
    for (size_t i = 0; i < c.sc.size(); ++i) table[i] = c.sc[i].geom;
    *ntable = (int)c.sc.size();
    return PT_OK;
}

int pt_test_sphere_cluster_sweep(const PtGeom *geoms, int ngeoms, uint64_t seed, int64_t rays, uint64_t *certified2, uint64_t *violations, float *info18) {
    NEED_GPU();
    if (!geoms || ngeoms < 2 || !certified2 || !violations || rays < 0) return fail(PT_ERR_INVALID, "pt_test_sphere_cluster_sweep: bad argument");
    SphereClusters c;
    PTCHECK(c.build(geoms, ngeoms, "pt_test_sphere_cluster_sweep"));
    std::vector<GeomDev> hs;
    for (const SphereCull &e : c.sc) hs.push_back(c.hg[e.geom]);
    WallBox hb[2];
    memset(hb, 0, sizeof hb);
    for (int g = 0; g < 2; ++g)
        for (int a = 0; a < 3; ++a) { hb[g].lo[a] = c.box[g][a]; hb[g].hi[a] = c.box[g][3 + a]; }
    F3 slo, shi;
    scene_extent(c.hg, slo, shi);
    if (info18) c.info(info18);
    DevBuf<GeomDev> ds;
    DevBuf<WallBox> db;
    Counters<3> cnt;
    PTCHECK(ds.upload(hs));
    PTCHECK(db.upload(hb, 2));
    PTCHECK(cnt.zero());
    const int per_thread = 64;
    PTCHECK(launch_wait(k_sweep_sphere_clusters, sweep_grid(rays, per_thread, kTestThreads, 1 << 22), 0, ds.p, (int)hs.size(), c.n0, db.p, c.omax, slo, shi,
                        seed, per_thread, cnt.at(0), cnt.at(2)));
    return cnt.read({certified2, certified2 + 1, violations});
}

int pt_test_sphere_group_sweep(const PtGeom *geoms, int ngeoms, uint64_t seed, int64_t rays, uint64_t *certified, uint64_t *violations, int32_t *ngroups) {
    NEED_GPU();
    if (!geoms || ngeoms < 2 || !certified || !violations || rays < 0) return fail(PT_ERR_INVALID, "pt_test_sphere_group_sweep: bad argument");
    // the groups exactly as pt_init builds them for this scene's spheres (one cluster: clusters only split the table in two before the grouping)
    std::vector<GeomDev> hg;
    std::vector<SphereCull> sc;
    PTCHECK(pack_sphere_cull(geoms, ngeoms, "pt_test_sphere_group_sweep", hg, sc));
    if (sc.size() < 2) return fail(PT_ERR_INVALID, "pt_test_sphere_group_sweep: fewer than two spheres");
    double kmax = 0.0;
    for (const SphereCull &e : sc) kmax = std::max(kmax, (double)e.cullK);
    const float sdir = std::nextafter((float)std::sqrt(1.0 / (1.0 - kmax)), INFINITY);
    const double ob = scene_origin_bound(geoms, ngeoms, hg);
    std::vector<SphereCull> groups;
    int n0 = 0, grpN0 = 0;
    build_sphere_groups(sc, n0, ob, sdir, groups, grpN0);
    const int ng = (int)(sc.size() / (size_t)kSphGroupSize);
    if (ngroups) *ngroups = ng;
    std::vector<GeomDev> hs;
    for (const SphereCull &e : sc) hs.push_back(hg[e.geom]);
    F3 slo, shi;
    scene_extent(hg, slo, shi);
    DevBuf<GeomDev> ds;
    DevBuf<SphereCull> dg;
    Counters<2> cnt;
    PTCHECK(ds.upload(hs));
    PTCHECK(dg.upload(groups));
    PTCHECK(cnt.zero());
    const int per_thread = 64;
    PTCHECK(launch_wait(k_sweep_sphere_groups, sweep_grid(rays, per_thread, kTestThreads, 1 << 22), 0, ds.p, (int)hs.size(), dg.p, ng, sdir,
                        std::nextafter((float)ob, 0.0f), slo, shi, seed, per_thread, cnt.at(0), cnt.at(1)));
    return cnt.read({certified, violations});
}

int pt_test_wall_box_sweep(const PtGeom *geoms, int ngeoms, uint64_t seed, int64_t rays, uint64_t *culled, uint64_t *violations) {
    NEED_GPU();
    if (!geoms || ngeoms < 1 || !culled || !violations || rays < 0) return fail(PT_ERR_INVALID, "pt_test_wall_box_sweep: bad argument");
    std::vector<GeomDev> hg;
    PTCHECK(pack_geoms(geoms, ngeoms, kCubes, nullptr, "pt_test_wall_box_sweep", hg));
    std::vector<WallBox> hw(ngeoms);
    std::vector<float> omax(ngeoms);
    for (int i = 0; i < ngeoms; ++i) {
        double om = 0;
        const double b = wall_box(geoms[i], hw[i], &om);
        if (b < 0) return fail(PT_ERR_INVALID, "pt_test_wall_box_sweep: cube %d is not finite", i);
        omax[i] = (float)om;                      // pt_init's bound, for a scene that consists of this wall alone
    }
    DevBuf<GeomDev> dg;
    DevBuf<WallBox> dw;
    DevBuf<float> dm;
    Counters<2> cnt;
    PTCHECK(dg.upload(hg));
    PTCHECK(dw.upload(hw));
    PTCHECK(dm.upload(omax));
    PTCHECK(cnt.zero());
    const int per_thread = 256;
    PTCHECK(launch_wait(k_sweep_wall_box, sweep_grid(rays, per_thread, kTestThreads, 1 << 20), 0, dg.p, dw.p, dm.p, ngeoms, seed, per_thread, cnt.at(0),
                        cnt.at(1)));
    return cnt.read({culled, violations});
}

int pt_test_slab_decisions(const PtGeom *cube, const float *rays, int n, uint32_t *flags, float *box7) {
    NEED_GPU();
    if (!cube || !rays || !flags || n < 0) return fail(PT_ERR_INVALID, "pt_test_slab_decisions: bad argument");
    std::vector<GeomDev> hg;
    PTCHECK(pack_geoms(cube, 1, kCubes, nullptr, "pt_test_slab_decisions", hg));
    std::vector<WallBox> hw(1);
    double om = 0;
    if (wall_box(cube[0], hw[0], &om) < 0) return fail(PT_ERR_INVALID, "pt_test_slab_decisions: the cube is not finite");
    const float omax = (float)om;
    if (box7) {
        for (int a = 0; a < 3; ++a) box7[a] = hw[0].lo[a], box7[3 + a] = hw[0].hi[a];
        box7[6] = omax;
    }
    if (n == 0) return PT_OK;
    DevBuf<GeomDev> dg;
    DevBuf<WallBox> dw;
    DevBuf<float> dr;
    DevBuf<uint32_t> df;
    PTCHECK(dg.upload(hg));
    PTCHECK(dw.upload(hw));
    PTCHECK(dr.upload(rays, (size_t)n * 6));
    PTCHECK(df.alloc(n));
    PTCHECK(launch_wait(k_test_slab_decisions, blocks_for(n), 0, dg.p, dw.p, omax, dr.p, n, df.p));
    return download(flags, df, n);
}

// host only: no GPU is touched
int pt_test_camera_cull_tables(const PtCamera *cam, const PtGeom *geoms, int ngeoms, int32_t *rects4, int32_t *scene_rect4, int32_t *spans2) {
    if (!cam || !geoms || ngeoms < 1 || !rects4 || !scene_rect4 || !spans2) return fail(PT_ERR_INVALID, "pt_test_camera_cull_tables: bad argument");
    CameraFixture f;
    PTCHECK(f.cull(cam, geoms, ngeoms, kAnyGeom, kAnyResolution, "pt_test_camera_cull_tables"));
    const std::vector<GeomDev> &hg = f.hg;
    const CameraCull &cc = f.cc;
    for (int i = 0; i < ngeoms; ++i)
        for (int a = 0; a < 4; ++a) rects4[4 * i + a] = hg[i].rect[a];
    for (int a = 0; a < 4; ++a) scene_rect4[a] = cc.sceneRect[a];
    for (int y = 0; y < f.k.H; ++y)
        for (int i = 0; i < ngeoms; ++i) {
            int x0 = 1, x1 = 0;                                // (empty: the row's list does not hold the primitive)
            if (cc.rowOff.empty()) { x0 = hg[i].rect[0]; x1 = hg[i].rect[2]; }
            else
                for (int e = cc.rowOff[y]; e < cc.rowOff[y + 1]; ++e)
                    if (cc.rowIdx[2 * e] == i) { x0 = cc.rowIdx[2 * e + 1] & 0xffff; x1 = cc.rowIdx[2 * e + 1] >> 16; }
            spans2[2 * ((size_t)y * ngeoms + i)] = x0;
            spans2[2 * ((size_t)y * ngeoms + i) + 1] = x1;
        }
    return PT_OK;
}

// what pt_test_camera_list and pt_test_camera_resolved hand out of a list (`face`: the resolved one's per-wave faces)
static void copy_camera_list(const CameraList &cl, uint32_t *pix, int32_t *wave2, int32_t *sig_idx, int32_t *face) {
    memcpy(pix, cl.pix.data(), cl.pix.size() * sizeof(uint32_t));
    memcpy(wave2, cl.wave.data(), cl.wave.size() * sizeof(int));
    memcpy(sig_idx, cl.sigIdx.data(), cl.sigIdx.size() * sizeof(int));
    if (face) memcpy(face, cl.face.data(), cl.face.size() * sizeof(int));
}

// host only: the camera rays' packed work list pt_init builds from the same tables (build_camera_list), for one shard, without a length cap
int pt_test_camera_list(const PtCamera *cam, const PtGeom *geoms, int ngeoms, int shard_rank, int shard_count, uint32_t *pix, int32_t *wave2,
                        int32_t *sig_idx, int64_t *sizes4) {
    if (!cam || !geoms || ngeoms < 1 || !sizes4) return fail(PT_ERR_INVALID, "pt_test_camera_list: bad argument");
    CameraFixture f;
    CameraList cl;
    bool built = false;
    PTCHECK(f.cull(cam, geoms, ngeoms, kAnyGeom, kAnyResolution, "pt_test_camera_list"));
    PTCHECK(f.list(geoms, shard_rank, shard_count, false, "pt_test_camera_list", cl, built));
    sizes4[0] = built ? (int64_t)cl.pix.size() : -1;
    sizes4[1] = (int64_t)cl.sigIdx.size();
    sizes4[2] = cl.listed;
    sizes4[3] = (int64_t)(f.k.H > shard_rank ? (f.k.H - shard_rank + shard_count - 1) / shard_count : 0) * f.k.W;
    if (built && pix && wave2 && sig_idx) copy_camera_list(cl, pix, wave2, sig_idx, nullptr);
    return PT_OK;
}

// host only: the list as pt_init builds it for the untextured forms, with the per-wave faces beside it; no length cap
int pt_test_camera_resolved(const PtCamera *cam, const PtGeom *geoms, int ngeoms, int shard_rank, int shard_count, uint32_t *pix, int32_t *wave2,
                            int32_t *sig_idx, int32_t *face, int64_t *sizes4) {
    if (!cam || !geoms || ngeoms < 1 || !sizes4) return fail(PT_ERR_INVALID, "pt_test_camera_resolved: bad argument");
    CameraFixture f;
    CameraList cl;
    bool built = false;
    PTCHECK(f.cull(cam, geoms, ngeoms, kAnyGeom, kAnyResolution, "pt_test_camera_resolved"));
    PTCHECK(f.list(geoms, shard_rank, shard_count, true, "pt_test_camera_resolved", cl, built));
    sizes4[0] = built ? (int64_t)cl.pix.size() : -1;
    sizes4[1] = (int64_t)cl.sigIdx.size();
    sizes4[2] = cl.listed;
    sizes4[3] = cl.resolved;
    if (built && pix && wave2 && sig_idx && face) copy_camera_list(cl, pix, wave2, sig_idx, face);
    return PT_OK;
}

// the same list with its certificates evaluated on the device between build_camera_list's two passes, as the camera move (pt_api.hip) evaluates them
// (k_camera_faces); kernel_ms (or NULL): the launches' time by HIP events
int pt_test_camera_resolved_device(const PtCamera *cam, const PtGeom *geoms, int ngeoms, int shard_rank, int shard_count, uint32_t *pix, int32_t *wave2,
                                   int32_t *sig_idx, int32_t *face, int64_t *sizes4, float *kernel_ms) {
    NEED_GPU();
    if (!cam || !geoms || ngeoms < 1 || !sizes4) return fail(PT_ERR_INVALID, "pt_test_camera_resolved_device: bad argument");
    if (shard_count < 1 || shard_rank < 0 || shard_rank >= shard_count) return fail(PT_ERR_INVALID, "pt_test_camera_resolved_device: bad shard");
    if (kernel_ms) *kernel_ms = 0.0f;
    CameraFixture f;
    CameraList cl;
    PTCHECK(f.cull(cam, geoms, ngeoms, kAnyGeom, kAnyResolution, "pt_test_camera_resolved_device"));
    CameraResolve cr;
    build_camera_resolve(geoms, f.k.ngeoms, f.k, f.hg, cr);
    CameraGroups G;
    const long long noCap = std::numeric_limits<long long>::max();
    const bool built = camera_list_groups(f.cc, f.k.W, f.k.H, shard_rank, shard_count, noCap, G);
    cl.listed = G.listed;
    if (built) {
        DevBuf<uint32_t> dpix;
        DevBuf<signed char> dface;
        PTCHECK(camera_faces_device(G, cr, nullptr, dpix, dface, kernel_ms));
        camera_list_emit(G, noCap, cl, &cr);
    }
    sizes4[0] = built ? (int64_t)cl.pix.size() : -1;
    sizes4[1] = (int64_t)cl.sigIdx.size();
    sizes4[2] = cl.listed;
    sizes4[3] = cl.resolved;
    if (built && pix && wave2 && sig_idx && face) copy_camera_list(cl, pix, wave2, sig_idx, face);
    return PT_OK;
}

// which way the calling thread's last camera move (pt_api.hip: set_camera) went: *fast 1 (every buffer kept) or 0 (pt_init inside), -1 before the first move and
// after a refusal; the tables the fast path uploaded and their bytes
int pt_test_last_camera_move(int *fast, int *tables_uploaded, int *bytes_uploaded) {
    if (!fast || !tables_uploaded || !bytes_uploaded) return fail(PT_ERR_INVALID, "pt_test_last_camera_move: bad argument");
    *fast = t_lastMove.fast;
    *tables_uploaded = t_lastMove.tables;
    *bytes_uploaded = (int)std::min<long long>(t_lastMove.bytes, std::numeric_limits<int>::max());
    return PT_OK;
}

// why the calling thread's last full pt_init call with PT_FLAG_KEEP_RENDERER did not move the camera in place (pt_api.hip: keep_mismatch): the name
// of the comparison that failed, "" where it matched or there has been no such call
int pt_test_keep_mismatch(char *why, int bytes) {
    if (!why || bytes < 1) return fail(PT_ERR_INVALID, "pt_test_keep_mismatch: bad argument");
    snprintf(why, (size_t)bytes, "%s", t_keepWhy ? t_keepWhy : "");
    return PT_OK;
}

int pt_test_face_hit_sweep(const PtCamera *cam, const PtGeom *geoms, int ngeoms, int samples, uint64_t seed, uint64_t counts[3]) {
    NEED_GPU();
    if (!cam || !geoms || ngeoms < 1 || samples < 0 || samples > 4096 || !counts) return fail(PT_ERR_INVALID, "pt_test_face_hit_sweep: bad argument");
    CameraFixture f;
    CameraList cl;
    bool built = false;
    PTCHECK(f.cull(cam, geoms, ngeoms, kAnyGeom, 1ll << 22, "pt_test_face_hit_sweep"));
    PTCHECK(f.list(geoms, 0, 1, true, "pt_test_face_hit_sweep", cl, built));
    if (!built) return fail(PT_ERR_INVALID, "pt_test_face_hit_sweep: no work list for this scene");
    std::vector<int> entries;
    for (size_t w = 0; w < cl.face.size(); ++w) {
        if (cl.face[w] < 0) continue;
        for (size_t l = 64 * w; l < 64 * w + 64; ++l)
            if (cl.pix[l] != kCamPad) { entries.push_back((int)cl.pix[l]); entries.push_back(cl.sigIdx[(size_t)cl.wave[2 * w]]); entries.push_back(cl.face[w]); }
    }
    counts[0] = counts[1] = 0;
    counts[2] = entries.size() / 3;
    if (entries.empty()) return PT_OK;
    const KParams &k = f.k;
    const float cam16[16] = {k.view[0], k.view[1], k.view[2], k.up[0], k.up[1], k.up[2], k.right[0], k.right[1], k.right[2],
                             k.pos[0], k.pos[1], k.pos[2], k.pixLenX, k.pixLenY, k.halfW, k.halfH};
    DevBuf<GeomDev> dg;
    DevBuf<float> dc;
    DevBuf<int> de;
    Counters<2> cnt;
    PTCHECK(dg.upload(f.hg));
    PTCHECK(dc.upload(cam16, 16));
    PTCHECK(de.upload(entries));
    PTCHECK(cnt.zero());
    // (one ray per lane, and lanes that stride over the rest where the cap cuts the grid: the kernel's streams are per ray)
    const long long total = (long long)(entries.size() / 3) * (samples + 4);
    PTCHECK(launch_wait(k_sweep_face_hit, sweep_grid(total, 1, kTestThreads, 1 << 16), 0, dg.p, dc.p, de.p, (int)(entries.size() / 3), samples, seed,
                        cnt.at(0)));
    return cnt.read({counts, counts + 1});
}

int pt_test_camera_cull_sweep(const PtCamera *cam, const PtGeom *geoms, int ngeoms, int samples, uint64_t *hits, uint64_t *culled,
                              uint64_t *violations) {
    NEED_GPU();
    if (!cam || !geoms || ngeoms < 1 || samples < 1 || !hits || !culled || !violations) return fail(PT_ERR_INVALID, "pt_test_camera_cull_sweep: bad argument");
    // exactly what pt_init derives: camera constants, packed primitives (object-space eye), rectangles, union, row lists
    CameraFixture f;
    PTCHECK(f.cull(cam, geoms, ngeoms, kSpheres | kCubes, 1ll << 26, "pt_test_camera_cull_sweep"));
    DevBuf<GeomDev> dg;
    DevBuf<int> doff, didx;
    Counters<3> cnt;
    PTCHECK(dg.upload(f.hg));
    if (!f.cc.rowOff.empty()) {
        PTCHECK(doff.upload(f.cc.rowOff));
        PTCHECK(didx.upload(f.cc.rowIdx));
    }
    PTCHECK(cnt.zero());
    PTCHECK(launch_wait(k_sweep_camera_cull, blocks_for(f.k.W * f.k.H), 0, f.k, dg.p, doff.p, didx.p, samples, cnt.at(0), cnt.at(1), cnt.at(2)));
    return cnt.read({hits, culled, violations});
}

int pt_test_camera_cull_margin(const PtCamera *cam, const PtGeom *geoms, int ngeoms, int samples, double *worst_fraction, uint64_t *needed) {
    NEED_GPU();
    if (!cam || !geoms || ngeoms < 1 || samples < 1 || !worst_fraction || !needed) return fail(PT_ERR_INVALID, "pt_test_camera_cull_margin: bad argument");
    CameraFixture f;
    PTCHECK(f.pack(cam, geoms, ngeoms, kSpheres | kCubes, 1ll << 26, "pt_test_camera_cull_margin"));
    std::vector<double> infl(4 * (size_t)ngeoms, 0.0);
    for (int i = 0; i < ngeoms; ++i) {
        double lo[3], hi[3];
        inflated_object_box(geoms[i], f.k.pos, nullptr, lo, hi);
        int rect[4];
        std::vector<std::pair<double, double>> hull;
        project_geom(geoms[i], f.k, rect, nullptr, &hull);
        for (int a = 0; a < 3; ++a) infl[4 * i + a] = geoms[i].type == PT_CUBE ? hi[a] - 0.5 : hi[0];
        infl[4 * i + 3] = hull.empty() ? 0.0 : 1.0;          // (culling switched off for this primitive: nothing to measure)
    }
    DevBuf<GeomDev> dg;
    DevBuf<double> di;
    Counters<2> cnt;
    PTCHECK(dg.upload(f.hg));
    PTCHECK(di.upload(infl));
    PTCHECK(cnt.zero());
    PTCHECK(launch_wait(k_sweep_camera_cull_margin, blocks_for(f.k.W * f.k.H), 0, f.k, dg.p, di.p, samples, cnt.at(0), cnt.at(1)));
    PTCHECK(cnt.read());
    memcpy(worst_fraction, &cnt.h[0], sizeof(double));
    *needed = cnt.h[1];
    return PT_OK;
}

int pt_test_wall_plane_sweep(const PtGeom *geoms, int ngeoms, uint64_t seed, int64_t rays, int32_t *nplane, uint64_t *certified,
                             uint64_t *violations, uint64_t *single) {
    NEED_GPU();
    if (!geoms || ngeoms < 1 || !nplane || !certified || !violations || !single || rays < 0) return fail(PT_ERR_INVALID, "pt_test_wall_plane_sweep: bad argument");
    std::vector<GeomDev> hg;
    KParams k;
    std::vector<WallBox> hw;
    std::vector<int> wallGeom;
    PTCHECK(test_choose_walls(geoms, ngeoms, "pt_test_wall_plane_sweep", hg, k, hw, wallGeom));
    *nplane = k.nSlotWalls + k.nPlaneWalls;
    *certified = *violations = *single = 0;
    if (k.nWalls < 1 || k.nSlotWalls + k.nPlaneWalls < 1) return PT_OK;
    std::vector<GeomDev> wg(k.nWalls);
    for (int w = 0; w < k.nWalls; ++w) wg[w] = hg[wallGeom[w]];
    DevBuf<GeomDev> dg;
    DevBuf<WallBox> dw;
    Counters<3> cnt;
    PTCHECK(dg.upload(wg));
    PTCHECK(dw.upload(hw.data(), k.nWalls));
    PTCHECK(cnt.zero());
    const int per_thread = 256;
    PTCHECK(launch_wait(k_sweep_wall_planes, sweep_grid(rays, per_thread, kTestThreads, 1 << 20), 0, k, dg.p, dw.p, seed, per_thread, cnt.at(0), cnt.at(1),
                        cnt.at(2)));
    return cnt.read({certified, violations, single});
}

// (host only) the inner face pt_init names per primitive of the scene -- 2 K + (s > 0) for a wall that has one, else -1 -- and the clearance
// that goes with it: plan_scene, no device (PT_AMD_NO_WALL_RESOLVE: every face -1)
int pt_test_wall_faces(const PtCamera *cam, const PtGeom *geoms, int ngeoms, const PtMaterial *mats, int nmats, int traceDepth, const PtOptions *opts,
                       int32_t *face, float *beyond) {
    if (!face || !beyond) return fail(PT_ERR_INVALID, "pt_test_wall_faces: bad argument");
    ScenePlan p;
    PTCHECK(plan_scene(SceneIn(cam, geoms, ngeoms, mats, nmats, traceDepth, effective_options(opts), R().reg), p));
    for (int i = 0; i < ngeoms; ++i) {
        const int w = (p.hg[(size_t)i].flags >> 2) & 7;                  // 1 + index among the walls, 0: not one
        face[i] = w != 0 ? p.hw[(size_t)w - 1].face : -1;
        beyond[i] = w != 0 ? p.hw[(size_t)w - 1].beyond : 0.0f;
    }
    return PT_OK;
}

int pt_test_wall_face_sweep(const PtGeom *geoms, int ngeoms, uint64_t seed, int64_t rays, uint64_t counts[4]) {
    NEED_GPU();
    if (!geoms || ngeoms < 1 || !counts || rays < 0) return fail(PT_ERR_INVALID, "pt_test_wall_face_sweep: bad argument");
    std::vector<GeomDev> hg;
    KParams k;
    std::vector<WallBox> hw;
    std::vector<int> wallGeom;
    PTCHECK(test_choose_walls(geoms, ngeoms, "pt_test_wall_face_sweep", hg, k, hw, wallGeom));
    choose_wall_faces(geoms, k, wallGeom, false, hw);
    for (int q = 0; q < 4; ++q) counts[q] = 0;
    std::vector<int> faced;
    for (int w = 0; w < k.nWalls; ++w)
        if (hw[(size_t)w].face >= 0) faced.push_back(w);
    if (faced.empty()) return PT_OK;
    // the room: per axis the innermost planes of the walls' (inflated) boxes on either side of the middle of the box around them all
    F3 lo = F3{k.outerLo[0], k.outerLo[1], k.outerLo[2]}, hi = F3{k.outerHi[0], k.outerHi[1], k.outerHi[2]};
    {
        float l[3] = {lo.x, lo.y, lo.z}, h[3] = {hi.x, hi.y, hi.z};
        for (int a = 0; a < 3; ++a) {
            const float mid = 0.5f * (l[a] + h[a]);
            float nl = l[a], nh = h[a];
            for (int w = 0; w < k.nWalls; ++w) {
                if (hw[(size_t)w].hi[a] < mid) nl = std::max(nl, hw[(size_t)w].hi[a]);
                if (hw[(size_t)w].lo[a] > mid) nh = std::min(nh, hw[(size_t)w].lo[a]);
            }
            l[a] = nl; h[a] = nh;
        }
        lo = F3{l[0], l[1], l[2]};
        hi = F3{h[0], h[1], h[2]};
    }
    std::vector<GeomDev> wg((size_t)k.nWalls);
    for (int w = 0; w < k.nWalls; ++w) wg[(size_t)w] = hg[(size_t)wallGeom[(size_t)w]];
    DevBuf<GeomDev> dg;
    DevBuf<WallBox> dw;
    DevBuf<int> df;
    Counters<4> cnt;
    PTCHECK(dg.upload(wg));
    PTCHECK(dw.upload(hw.data(), (size_t)k.nWalls));
    PTCHECK(df.upload(faced));
    PTCHECK(cnt.zero());
    const int per_thread = 64;
    PTCHECK(launch_wait(k_sweep_wall_face, sweep_grid(rays, per_thread, kTestThreads, 1 << 20), 0, dg.p, dw.p, df.p, (int)faced.size(), lo, hi, seed, per_thread,
                        cnt.at(0)));
    return cnt.read({counts, counts + 1, counts + 2, counts + 3});
}

// the test library's tally of the later bounces' resolved one-wall tiles (ptd::g_wallResolve), read and cleared
int pt_test_wall_resolve_tally(uint64_t counts[4]) {
    NEED_GPU();
    if (!counts) return fail(PT_ERR_INVALID, "pt_test_wall_resolve_tally: bad argument");
    unsigned long long h[4], z[4] = {0, 0, 0, 0};
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpyFromSymbol(h, HIP_SYMBOL(ptd::g_wallResolve), sizeof h));
    HIPCHECK(hipMemcpyToSymbol(HIP_SYMBOL(ptd::g_wallResolve), z, sizeof z));
    for (int q = 0; q < 4; ++q) counts[q] = h[q];
    return PT_OK;
}

// ... and of the later bounces' candidate tiles and the scatters' candidacy (ptd::g_candidates), read and cleared
int pt_test_candidate_tally(uint64_t counts[8]) {
    NEED_GPU();
    if (!counts) return fail(PT_ERR_INVALID, "pt_test_candidate_tally: bad argument");
    unsigned long long h[8], z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpyFromSymbol(h, HIP_SYMBOL(ptd::g_candidates), sizeof h));
    HIPCHECK(hipMemcpyToSymbol(HIP_SYMBOL(ptd::g_candidates), z, sizeof z));
    for (int q = 0; q < 8; ++q) counts[q] = h[q];
    return PT_OK;
}

// ... and of the grouped sweep of the later bounces (ptd::g_groupSweep), read and cleared
int pt_test_group_tally(uint64_t counts[6]) {
    NEED_GPU();
    if (!counts) return fail(PT_ERR_INVALID, "pt_test_group_tally: bad argument");
    unsigned long long h[6], z[6] = {0, 0, 0, 0, 0, 0};
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpyFromSymbol(h, HIP_SYMBOL(ptd::g_groupSweep), sizeof h));
    HIPCHECK(hipMemcpyToSymbol(HIP_SYMBOL(ptd::g_groupSweep), z, sizeof z));
    for (int q = 0; q < 6; ++q) counts[q] = h[q];
    return PT_OK;
}

int pt_test_box_fast_sweep(const PtGeom *geoms, int ngeoms, uint64_t seed, int64_t rays, uint64_t counts[4], uint64_t div_mismatches[2]) {
    NEED_GPU();
    if (!geoms || ngeoms < 1 || !counts || !div_mismatches || rays < 0) return fail(PT_ERR_INVALID, "pt_test_box_fast_sweep: bad argument");
    std::vector<GeomDev> hg;
    PTCHECK(pack_geoms(geoms, ngeoms, kCubes, nullptr, "pt_test_box_fast_sweep", hg));
    DevBuf<GeomDev> dg;
    DevBuf<float> dump;
    Counters<8> cnt;                                      // (0 .. 3: the box sweep's, 4 .. 5: the division's, 6: mismatching rays dumped)
    PTCHECK(dg.upload(hg));
    PTCHECK(cnt.zero());
    const bool verbose = env_flag("PT_AMD_VERBOSE");
    if (verbose) PTCHECK(dump.alloc(8 * 24));
    const int per_thread = 256;
    PTCHECK(launch_wait(k_sweep_box_fast, sweep_grid(rays, per_thread, kTestThreads, 1 << 20), 0, dg.p, ngeoms, seed, per_thread, cnt.at(0),
                        verbose ? dump.p : nullptr));
    PTCHECK(launch_wait(k_sweep_div_unscaled, dim3(1 << 12), 0, seed, 1024, cnt.at(4)));   // 2^20 threads
    PTCHECK(cnt.read({counts, counts + 1, counts + 2, counts + 3, div_mismatches, div_mismatches + 1}));
    if (verbose && cnt.h[6]) {                            // (experiments: the first mismatching rays)
        float r[8 * 24];
        PTCHECK(download(r, dump, 8 * 24));
        for (int i = 0; i < (int)std::min<unsigned long long>(cnt.h[6], 8); ++i) {
            const float *q = r + 24 * i;
            fprintf(stderr, "box sweep mismatch: geom %d org %.9g %.9g %.9g dir %.9g %.9g %.9g | t fast %.9g exact %.9g early %.9g outside %g %g | P %.9g %.9g %.9g / %.9g %.9g %.9g | n %a %a %a / %a %a %a\n",
                    (int)q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10], q[11], q[12], q[13], q[14], q[15], q[16], q[17], q[18], q[19], q[20], q[21], q[22], q[23]);
        }
    }
    return PT_OK;
}

int pt_test_slab_quotients(const float *o, const float *d, int n, float *t1, float *t2, float *ref1, float *ref2) {
    NEED_GPU();
    if (n <= 0) return PT_OK;
    DevBuf<float> a, b, q1, q2, r1, r2;
    PTCHECK(a.upload(o, n));
    PTCHECK(b.upload(d, n));
    PTCHECK(q1.alloc(n));
    PTCHECK(q2.alloc(n));
    PTCHECK(r1.alloc(n));
    PTCHECK(r2.alloc(n));
    PTCHECK(launch_wait(k_test_slab_quotients, blocks_for(n), 0, a.p, b.p, n, q1.p, q2.p, r1.p, r2.p));
    PTCHECK(download(t1, q1, n));
    PTCHECK(download(t2, q2, n));
    PTCHECK(download(ref1, r1, n));
    return download(ref2, r2, n);
}

int pt_test_slab_quotients_sweep(uint64_t seed, int64_t pairs, uint64_t *mismatches) {
    NEED_GPU();
    if (!mismatches || pairs < 0) return fail(PT_ERR_INVALID, "pt_test_slab_quotients_sweep: bad argument");
    Counters<1> cnt;
    PTCHECK(cnt.zero());
    const int per_thread = 1024;
    PTCHECK(launch_wait(k_sweep_slab_quotients, sweep_grid(pairs, per_thread, kTestThreads, 1 << 20), 0, seed, per_thread, cnt.at(0)));
    return cnt.read({mismatches});
}

int pt_test_unscaled_sqrt_sweep(uint64_t mismatches[4]) {
    NEED_GPU();
    if (!mismatches) return fail(PT_ERR_INVALID, "pt_test_unscaled_sqrt_sweep: bad argument");
    Counters<4> cnt;
    PTCHECK(cnt.zero());
    PTCHECK(launch_wait(k_sweep_unscaled_sqrt, dim3(1 << 14), 0, cnt.at(0)));   // 2^22 threads x 2^10 patterns
    return cnt.read({mismatches, mismatches + 1, mismatches + 2, mismatches + 3});
}

#ifdef PT_PROBE_TIMELINE
// instrumented build only (make timeline): reads and clears the per-phase cycle sums of pt_device.h
extern "C" int pt_probe_timeline(uint64_t out[128]) {      // [0, 64) cycles (later bounces, then + 32 the camera-ray bounce), [64, 128) intervals
    NEED_GPU();
    unsigned long long h[128], z[64] = {0};
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpyFromSymbol(h, HIP_SYMBOL(ptd::g_phaseT), 64 * sizeof(unsigned long long)));
    HIPCHECK(hipMemcpyFromSymbol(h + 64, HIP_SYMBOL(ptd::g_phaseN), 64 * sizeof(unsigned long long)));
    HIPCHECK(hipMemcpyToSymbol(HIP_SYMBOL(ptd::g_phaseT), z, sizeof z));
    HIPCHECK(hipMemcpyToSymbol(HIP_SYMBOL(ptd::g_phaseN), z, sizeof z));
    for (int i = 0; i < 128; ++i) out[i] = h[i];
    return PT_OK;
}
#elif defined(PT_PROBE)
// instrumented build only (make probe): the residency census of k_bounce -- out[k] = number of CUs on which at most k
// workgroups of it were ever resident together (k = 0..15); cleared by the call
extern "C" int pt_probe_census(uint32_t out[16]) {
    NEED_GPU();
    static unsigned int h[4096], z[4096];
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpyFromSymbol(h, HIP_SYMBOL(ptd::g_censusMax), sizeof h));
    HIPCHECK(hipMemcpyToSymbol(HIP_SYMBOL(ptd::g_censusMax), z, sizeof z));
    for (int k = 0; k < 16; ++k) out[k] = 0;
    for (int i = 0; i < 4096; ++i)
        if (h[i]) out[h[i] < 15 ? h[i] : 15]++;
    return PT_OK;
}
// instrumented build only (make probe): reads and clears the phase counters of pt_device.h
extern "C" int pt_probe_read(uint64_t out[64]) {
    NEED_GPU();
    unsigned long long h[64], z[64] = {0};
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpyFromSymbol(h, HIP_SYMBOL(ptd::g_probe), sizeof h));
    HIPCHECK(hipMemcpyToSymbol(HIP_SYMBOL(ptd::g_probe), z, sizeof z));
    for (int i = 0; i < 64; ++i) out[i] = h[i];
    return PT_OK;
}
#endif

int pt_test_hemisphere(const float *normals3, const int32_t *iid3, int n, float *out3) {
    NEED_GPU();
    if (n <= 0) return PT_OK;
    DevBuf<float> a, o;
    DevBuf<int> b;
    PTCHECK(a.upload(normals3, (size_t)n * 3));
    PTCHECK(b.upload(iid3, (size_t)n * 3));
    PTCHECK(o.alloc((size_t)n * 3));
    PTCHECK(launch_wait(k_test_hemisphere, blocks_for(n), 0, a.p, b.p, n, o.p));
    return download(out3, o, (size_t)n * 3);
}

int pt_test_pow(const float *x, const float *e, int n, float *out) {
    NEED_GPU();
    if (n <= 0) return PT_OK;
    DevBuf<float> a, b, o;
    PTCHECK(a.upload(x, n));
    PTCHECK(b.upload(e, n));
    PTCHECK(o.alloc(n));
    PTCHECK(launch_wait(k_test_pow, blocks_for(n), 0, a.p, b.p, n, o.p));
    return download(out, o, n);
}

int pt_test_exp_neg_poly(const float *a, int n, float *out) {
    NEED_GPU();
    if (n <= 0) return PT_OK;
    DevBuf<float> x, o;
    PTCHECK(x.upload(a, n));
    PTCHECK(o.alloc(n));
    PTCHECK(launch_wait(k_test_exp_neg_poly, blocks_for(n), 0, x.p, n, o.p));
    return download(out, o, n);
}

int pt_test_denoise(int samples, const PtDenoiseParams *p, size_t params_struct_bytes, int form, float *rgb_mean_host, float *ms) {
    return denoise_to_host(samples, p, params_struct_bytes, form, ms, rgb_mean_host, "pt_test_denoise");
}

int pt_test_denoise_var(int samples, const PtDenoiseVarParams *p, size_t params_struct_bytes, int form, float *rgb_mean_host, float *var_host, float *ms) {
    return denoise_var_to_host(samples, p, params_struct_bytes, form, ms, rgb_mean_host, var_host, "pt_test_denoise_var");
}

int pt_test_display(int samples, int form, int fused, void *rgba8_dev, float *ms) {
    PTCHECK(moments_refusals("pt_test_display"));
    if (!rgba8_dev || samples < 1 || (fused != 0 && fused != 1)) return fail(PT_ERR_INVALID, "pt_test_display: bad argument");
    if (ms) std::fill(ms, ms + 1 + PT_DISPLAY_LEVELS, 0.0f);
    return display_bytes(samples, reinterpret_cast<uchar4 *>(rgba8_dev), "pt_test_display", form, fused != 0, ms);
}

static_assert(sizeof(TemporalCam) == 16 * sizeof(float), "pt_test_temporal's cam16 is a TemporalCam (include/pt_amd_test.h)");

int pt_test_temporal_camera(const PtCamera *cam, float *cam16) {
    if (!cam || !cam16 || cam->resolution[0] < 1 || cam->resolution[1] < 1) return fail(PT_ERR_INVALID, "pt_test_temporal_camera: bad argument");
    KParams k{};
    camera_params(*cam, k);
    const TemporalCam c = temporal_camera(k);
    memcpy(cam16, &c, sizeof c);
    return PT_OK;
}

int pt_test_temporal(int capture, int w, int h, int samples, const float *rgb_sum, const float *lum_sq_sum, const float *pos_t4, const float *nrm_id4,
                     const float *hc4, const float *hn, const float *hpos_t4, const float *hnrm_id4, const float *cam16, float *out4, float *out_n,
                     int reps, float *ms) {
    NEED_GPU();
    if (capture < 0 || capture > 2 || w < 1 || h < 1 || (long long)w * h > (1ll << 30) || samples < 1 || !rgb_sum || !lum_sq_sum || !pos_t4 || !nrm_id4 || !hc4 || !hn || !hpos_t4 ||
        !hnrm_id4 || !cam16 || !out4 || (capture && !out_n) || (ms && reps < 1))
        return fail(PT_ERR_INVALID, "pt_test_temporal: bad argument");
    const size_t P = (size_t)w * h;
    DevBuf<float> S, Q, Hn, outN;
    DevBuf<float4> pos, nrm, Hc, Hpos, Hnrm, out;
    PTCHECK(S.upload(rgb_sum, P * 3));
    PTCHECK(Q.upload(lum_sq_sum, P));
    PTCHECK(Hn.upload(hn, P));
    PTCHECK(pos.upload(reinterpret_cast<const float4 *>(pos_t4), P));
    PTCHECK(nrm.upload(reinterpret_cast<const float4 *>(nrm_id4), P));
    PTCHECK(Hc.upload(reinterpret_cast<const float4 *>(hc4), P));
    PTCHECK(Hpos.upload(reinterpret_cast<const float4 *>(hpos_t4), P));
    PTCHECK(Hnrm.upload(reinterpret_cast<const float4 *>(hnrm_id4), P));
    int rc = out.alloc(P); if (rc) return rc;
    rc = outN.alloc(P); if (rc) return rc;
    TemporalArgs T;
    T.accum = S.p; T.moments = Q.p; T.posT = pos.p; T.nrmId = nrm.p;
    T.hc = Hc.p; T.hn = Hn.p; T.hpos = Hpos.p; T.hnrm = Hnrm.p;
    memcpy(&T.cam, cam16, sizeof T.cam);
    T.W = w; T.H = h; T.samples = (float)samples;
    T.out = out.p; T.outN = outN.p;
    const dim3 grid((unsigned)((P + kBlock - 1) / kBlock));
    PTCHECK(timed_launches(reps, ms, [&]() -> int {
        if (capture == 2) hipLaunchKernelGGL(k_temporal<kTemporalMoments>, grid, dim3(kBlock), 0, nullptr, T);
        else if (capture) hipLaunchKernelGGL(k_temporal<kTemporalCapture>, grid, dim3(kBlock), 0, nullptr, T);
        else hipLaunchKernelGGL(k_temporal<kTemporalFilter>, grid, dim3(kBlock), 0, nullptr, T);
        return PT_OK;
    }));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(out4, out.p, P * sizeof(float4), hipMemcpyDeviceToHost));
    if (capture) PTCHECK(download(out_n, outN, P));
    return PT_OK;
}

int pt_test_spatial_variance(int radius, int form, int w, int h, const float *m4, const float *n, const float *pos_t4, const float *nrm_id4,
                             float sigma_normal, float sigma_position, float *out4, int reps, float *ms) {
    NEED_GPU();
    if (radius < 1 || radius > 3 || (form != kSpatialGather && form != kSpatialTiled) || w < 1 || h < 1 || (long long)w * h > (1ll << 30) || !m4 || !n ||
        !pos_t4 || !nrm_id4 || !(sigma_normal > 0.0f) || !(sigma_position > 0.0f) || !out4 || (ms && reps < 1))
        return fail(PT_ERR_INVALID, "pt_test_spatial_variance: bad argument");
    const size_t P = (size_t)w * h;
    DevBuf<float> N;
    DevBuf<float4> M, pos, nrm, out;
    PTCHECK(M.upload(reinterpret_cast<const float4 *>(m4), P));
    PTCHECK(N.upload(n, P));
    PTCHECK(pos.upload(reinterpret_cast<const float4 *>(pos_t4), P));
    PTCHECK(nrm.upload(reinterpret_cast<const float4 *>(nrm_id4), P));
    int rc = out.alloc(P); if (rc) return rc;
    SpatialArgs A;
    A.m4 = M.p; A.cnt = N.p; A.posT = pos.p; A.nrmId = nrm.p;
    A.W = w; A.H = h;
    A.invN = 1.0f / (sigma_normal * sigma_normal);
    A.invP = 1.0f / (sigma_position * sigma_position);
    A.out = out.p;
    PTCHECK(timed_launches(reps, ms, [&] { return spatial_launch(A, radius, form, nullptr); }));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(out4, out.p, P * sizeof(float4), hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_test_albedo(float *asum4_host) {
    if (!R().init) return fail(PT_ERR_NOT_INIT, "pt_test_albedo before pt_init");
    if (!R().albedo.p) return fail(PT_ERR_INVALID, "pt_test_albedo: the renderer was initialised without PT_FLAG_DEMODULATE");
    if (!asum4_host) return fail(PT_ERR_INVALID, "pt_test_albedo: null");
    HIPCHECK(hipMemcpyAsync(asum4_host, R().albedo.p, (size_t)R().P * sizeof(float4), hipMemcpyDeviceToHost, R().stream));
    HIPCHECK(hipStreamSynchronize(R().stream));
    return readback_fault();
}

int pt_test_demodulate(int form, int inplace, int bytes, int w, int h, int samples, int levels, const float *rgb_sum, const float *lum_sq_sum, const float *img4,
                       const float *asum4, const float *pos_t4, const float *nrm_id4, float sigma_lum, float sigma_normal, float sigma_position,
                       float min_albedo, float *demod4_out, float *rgb_out, float *var_out, uint8_t *rgba_out, int reps, float *ms) {
    NEED_GPU();
    if (form < kAtrousGather || form > kAtrousTiled8 || (inplace != 0 && inplace != 1) || (bytes != 0 && bytes != 1) || w < 1 || h < 1 ||
        (long long)w * h > (1ll << 30) || samples < (inplace ? 1 : 2) || levels < 1 || levels > 8 || (inplace ? !img4 : (!rgb_sum || !lum_sq_sum)) || !asum4 ||
        !pos_t4 || !nrm_id4 || !(sigma_lum > 0.0f) || !(sigma_normal > 0.0f) || !(sigma_position > 0.0f) || !(min_albedo > 0.0f) ||
        (bytes ? !rgba_out : !rgb_out) || (ms && reps < 1))
        return fail(PT_ERR_INVALID, "pt_test_demodulate: bad argument");
    const size_t P = (size_t)w * h;
    DevBuf<float> S, Q, out3, outVar;
    DevBuf<float4> ping[2], asum, pos, nrm;
    DevBuf<uchar4> out8;
    if (inplace) {
        PTCHECK(ping[1].upload(reinterpret_cast<const float4 *>(img4), P));
    } else {
        PTCHECK(S.upload(rgb_sum, P * 3));
        PTCHECK(Q.upload(lum_sq_sum, P));
        PTCHECK(ping[1].alloc(P));
    }
    PTCHECK(ping[0].alloc(P));
    PTCHECK(asum.upload(reinterpret_cast<const float4 *>(asum4), P));
    PTCHECK(pos.upload(reinterpret_cast<const float4 *>(pos_t4), P));
    PTCHECK(nrm.upload(reinterpret_cast<const float4 *>(nrm_id4), P));
    if (bytes) {
        PTCHECK(out8.alloc(P));
    } else {
        PTCHECK(out3.alloc(P * 3));
        if (var_out) PTCHECK(outVar.alloc(P));
    }
    DemodArgs D;
    D.accum = S.p; D.moments = Q.p; D.img = ping[1].p; D.asum = asum.p;
    D.npix = (int)P;
    D.samples = (float)samples; D.samplesM1 = (float)(samples - 1); D.eps = min_albedo;
    AtrousDemodArgs A;
    A.accum = nullptr; A.moments = nullptr;
    A.outVar = outVar.p;
    A.posT = pos.p; A.nrmId = nrm.p;
    A.W = w; A.H = h;
    A.samples = (float)samples; A.samplesM1 = (float)(samples - 1);
    A.invN = 1.0f / (sigma_normal * sigma_normal);
    A.invP = 1.0f / (sigma_position * sigma_position);
    A.asum = asum.p; A.demodN = (float)samples; A.demodEps = min_albedo;
    Event ev[4];
    if (ms) for (Event &e : ev) PTCHECK(e.create(hipEventDefault));
    for (int r = 0; r < (ms ? reps + 1 : 1); ++r) {           // (timed: one untimed run first)
        if (ms && r) HIPCHECK(hipEventRecord(ev[0], nullptr));
        PTCHECK(demod_launch(D, inplace != 0, nullptr));
        if (ms && r) HIPCHECK(hipEventRecord(ev[1], nullptr));
        if (r == 0 && demod4_out) HIPCHECK(hipMemcpy(demod4_out, ping[1].p, P * sizeof(float4), hipMemcpyDeviceToHost));
        for (int i = 0; i < levels; ++i) {
            const bool last = i == levels - 1;
            A.step = 1 << i;
            AtrousGuided::hostColourScale(A, sigma_lum, i);
            A.cin = ping[(i + 1) & 1].p;
            A.cout = last ? nullptr : ping[i & 1].p;
            A.out3 = nullptr;
            if (last && bytes) A.out8 = out8.p;
            else if (last) A.out3 = out3.p;
            int f = form;
            unsigned long long grid = f == kAtrousGather ? atrousGridGather(w, h) : atrousGridTiled(w, h, A.step, f == kAtrousTiled4 ? 1 : 2);
            if (grid > 0x7fffffffull) {
                f = kAtrousGather;
                grid = atrousGridGather(w, h);
            }
            void *kargs[] = {&A};
            if (ms && r && last) HIPCHECK(hipEventRecord(ev[2], nullptr));
            HIPCHECK(hipLaunchKernel(last ? atrous_last_kernel<AtrousDemod>(bytes != 0, f) : atrous_kernel<AtrousGuided>(false, false, false, f), dim3((unsigned)grid),
                                     dim3(kBlock), kargs, 0, nullptr));
        }
        if (ms && r) {
            HIPCHECK(hipEventRecord(ev[3], nullptr));
            HIPCHECK(hipEventSynchronize(ev[3]));
            HIPCHECK(hipEventElapsedTime(&ms[2 * (r - 1)], ev[0], ev[1]));
            HIPCHECK(hipEventElapsedTime(&ms[2 * (r - 1) + 1], ev[2], ev[3]));
        }
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    if (bytes) {
        HIPCHECK(hipMemcpy(rgba_out, out8.p, P * 4, hipMemcpyDeviceToHost));
    } else {
        PTCHECK(download(rgb_out, out3, P * 3));
        if (var_out) PTCHECK(download(var_out, outVar, P));
    }
    return PT_OK;
}

int pt_test_history(int32_t *wh2, float *hc4, float *hn, float *hpos_t4, float *hnrm_id4, float *cam16) {
    if (!wh2) return fail(PT_ERR_INVALID, "pt_test_history: null");
    const History &hs = R().hist;
    wh2[0] = hs.live ? hs.W : 0;
    wh2[1] = hs.live ? hs.H : 0;
    if (!hs.live) return PT_OK;
    const size_t P = (size_t)hs.W * hs.H;
    if (hc4) HIPCHECK(hipMemcpy(hc4, hs.hc[hs.cur].p, P * sizeof(float4), hipMemcpyDeviceToHost));
    if (hn) HIPCHECK(hipMemcpy(hn, hs.hn[hs.cur].p, P * sizeof(float), hipMemcpyDeviceToHost));
    if (hpos_t4) HIPCHECK(hipMemcpy(hpos_t4, hs.hpos.p, P * sizeof(float4), hipMemcpyDeviceToHost));
    if (hnrm_id4) HIPCHECK(hipMemcpy(hnrm_id4, hs.hnrm.p, P * sizeof(float4), hipMemcpyDeviceToHost));
    if (cam16) memcpy(cam16, &hs.cam, sizeof hs.cam);
    return PT_OK;
}

int pt_test_history_albedo(int32_t *wh2, float *ha4) {
    if (!wh2) return fail(PT_ERR_INVALID, "pt_test_history_albedo: null");
    const History &hs = R().hist;
    const bool has = hs.live && hs.albedo;
    wh2[0] = has ? hs.W : 0;
    wh2[1] = has ? hs.H : 0;
    if (!has) return PT_OK;
    if (ha4) HIPCHECK(hipMemcpy(ha4, hs.ha[hs.cur].p, (size_t)hs.W * hs.H * sizeof(float4), hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_test_temporal_albedo(int form, int front, int w, int h, int samples, const float *rgb_sum, const float *lum_sq_sum, const float *pos_t4,
                            const float *nrm_id4, const float *asum4, const float *hc4, const float *hn, const float *ha4, const float *hpos_t4,
                            const float *hnrm_id4, const float *cam16, float min_albedo, float *out4, float *out_n, float *out_a4, int reps, float *ms) {
    NEED_GPU();
    if (form < 0 || form > 2 || front < 0 || front > 2 || (form != 0 && front != 0) || w < 1 || h < 1 || (long long)w * h > (1ll << 30) || samples < 1 ||
        !rgb_sum || !lum_sq_sum || !pos_t4 || !nrm_id4 || !asum4 || !hc4 || !hn || !ha4 || !hpos_t4 || !hnrm_id4 || !cam16 || !(min_albedo > 0.0f) || !out4 ||
        (form && !out_n) || !out_a4 || (ms && reps < 1))
        return fail(PT_ERR_INVALID, "pt_test_temporal_albedo: bad argument");
    const size_t P = (size_t)w * h;
    DevBuf<float> S, Q, Hn, outN;
    DevBuf<float4> pos, nrm, Asum, Hc, Ha, Hpos, Hnrm, out, outA;
    PTCHECK(S.upload(rgb_sum, P * 3));
    PTCHECK(Q.upload(lum_sq_sum, P));
    PTCHECK(Hn.upload(hn, P));
    PTCHECK(pos.upload(reinterpret_cast<const float4 *>(pos_t4), P));
    PTCHECK(nrm.upload(reinterpret_cast<const float4 *>(nrm_id4), P));
    PTCHECK(Asum.upload(reinterpret_cast<const float4 *>(asum4), P));
    PTCHECK(Hc.upload(reinterpret_cast<const float4 *>(hc4), P));
    PTCHECK(Ha.upload(reinterpret_cast<const float4 *>(ha4), P));
    PTCHECK(Hpos.upload(reinterpret_cast<const float4 *>(hpos_t4), P));
    PTCHECK(Hnrm.upload(reinterpret_cast<const float4 *>(hnrm_id4), P));
    PTCHECK(out.alloc(P));
    PTCHECK(outN.alloc(P));
    PTCHECK(outA.alloc(P));
    TemporalArgs T;
    T.accum = S.p; T.moments = Q.p; T.posT = pos.p; T.nrmId = nrm.p;
    T.hc = Hc.p; T.hn = Hn.p; T.hpos = Hpos.p; T.hnrm = Hnrm.p;
    memcpy(&T.cam, cam16, sizeof T.cam);
    T.W = w; T.H = h; T.samples = (float)samples;
    T.out = out.p; T.outN = outN.p;
    T.ha = Ha.p; T.asum = Asum.p; T.outA = outA.p; T.eps = min_albedo;
    DemodArgs D;
    D.accum = nullptr; D.moments = nullptr; D.img = out.p; D.asum = outA.p;
    D.npix = (int)P;
    D.samples = 1.0f; D.samplesM1 = 0.0f; D.eps = min_albedo;
    const dim3 grid((unsigned)((P + kBlock - 1) / kBlock));
    PTCHECK(timed_launches(reps, ms, [&]() -> int {
        if (form == 2) hipLaunchKernelGGL((k_temporal<kTemporalMoments, true>), grid, dim3(kBlock), 0, nullptr, T);
        else if (form == 1) hipLaunchKernelGGL((k_temporal<kTemporalCapture, true>), grid, dim3(kBlock), 0, nullptr, T);
        else if (front == 1) hipLaunchKernelGGL((k_temporal<kTemporalFilterDemod, true>), grid, dim3(kBlock), 0, nullptr, T);
        else hipLaunchKernelGGL((k_temporal<kTemporalFilter, true>), grid, dim3(kBlock), 0, nullptr, T);
        return front == 2 ? demod_launch(D, true, nullptr) : (int)PT_OK;
    }));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(out4, out.p, P * sizeof(float4), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(out_a4, outA.p, P * sizeof(float4), hipMemcpyDeviceToHost));
    if (form) PTCHECK(download(out_n, outN, P));
    return PT_OK;
}

int pt_test_motion_table(const PtGeom *then, const PtGeom *now, int ngeoms, float *rows24, int32_t *any) {
    if (!then || !now || ngeoms < 1 || !rows24 || !any) return fail(PT_ERR_INVALID, "pt_test_motion_table: bad argument");
    std::vector<MotionRow> rows;
    *any = motion_table(then, now, ngeoms, rows) ? 1 : 0;
    memcpy(rows24, rows.data(), rows.size() * sizeof(MotionRow));
    return PT_OK;
}

int pt_test_history_motion(int32_t *nrows, float *rows24, float *cap) {
    if (!nrows) return fail(PT_ERR_INVALID, "pt_test_history_motion: null");
    const History &hs = R().hist;
    const bool has = hs.live && hs.motion.p;
    *nrows = has ? (int32_t)hs.motionHost.size() : 0;
    if (cap) *cap = hs.cap;
    if (!has) return PT_OK;
    // (the device's bytes: what the kernels read)
    if (rows24) HIPCHECK(hipMemcpy(rows24, hs.motion.p, hs.motionHost.size() * sizeof(MotionRow), hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_test_temporal_motion(int form, int albedo, int motion, int w, int h, int samples, const float *rgb_sum, const float *lum_sq_sum,
                            const float *pos_t4, const float *nrm_id4, const float *asum4, const float *hc4, const float *hn, const float *ha4,
                            const float *hpos_t4, const float *hnrm_id4, const float *cam16, const float *rows24, int nrows, float hist_cap,
                            float min_albedo, float *out4, float *out_n, float *out_a4, int reps, float *ms) {
    NEED_GPU();
    const bool needN = form == 1 || form == 2;
    if (form < 0 || form > 3 || (albedo != 0 && albedo != 1) || (motion != 0 && motion != 1) || (form == 3 && !albedo) || w < 1 || h < 1 ||
        (long long)w * h > (1ll << 30) || samples < 1 || !rgb_sum || !lum_sq_sum || !pos_t4 || !nrm_id4 || !hc4 || !hn || !hpos_t4 || !hnrm_id4 || !cam16 ||
        !out4 || (needN && !out_n) || (albedo && (!asum4 || !ha4 || !out_a4 || !(min_albedo > 0.0f))) || (motion && (!rows24 || nrows < 1 || nrows > (1 << 24))) ||
        (ms && reps < 1))
        return fail(PT_ERR_INVALID, "pt_test_temporal_motion: bad argument");
    const size_t P = (size_t)w * h;
    DevBuf<float> S, Q, Hn, outN;
    DevBuf<float4> pos, nrm, Asum, Hc, Ha, Hpos, Hnrm, out, outA, rows;
    PTCHECK(S.upload(rgb_sum, P * 3));
    PTCHECK(Q.upload(lum_sq_sum, P));
    PTCHECK(Hn.upload(hn, P));
    PTCHECK(pos.upload(reinterpret_cast<const float4 *>(pos_t4), P));
    PTCHECK(nrm.upload(reinterpret_cast<const float4 *>(nrm_id4), P));
    PTCHECK(Hc.upload(reinterpret_cast<const float4 *>(hc4), P));
    PTCHECK(Hpos.upload(reinterpret_cast<const float4 *>(hpos_t4), P));
    PTCHECK(Hnrm.upload(reinterpret_cast<const float4 *>(hnrm_id4), P));
    if (albedo) {
        PTCHECK(Asum.upload(reinterpret_cast<const float4 *>(asum4), P));
        PTCHECK(Ha.upload(reinterpret_cast<const float4 *>(ha4), P));
        PTCHECK(outA.alloc(P));
    }
    if (motion) PTCHECK(rows.upload(reinterpret_cast<const float4 *>(rows24), (size_t)nrows * kMotionRowVec));
    PTCHECK(out.alloc(P));
    PTCHECK(outN.alloc(P));
    TemporalArgs T;
    T.accum = S.p; T.moments = Q.p; T.posT = pos.p; T.nrmId = nrm.p;
    T.hc = Hc.p; T.hn = Hn.p; T.hpos = Hpos.p; T.hnrm = Hnrm.p;
    memcpy(&T.cam, cam16, sizeof T.cam);
    T.W = w; T.H = h; T.samples = (float)samples;
    T.out = out.p; T.outN = outN.p;
    T.ha = Ha.p; T.asum = Asum.p; T.outA = outA.p; T.eps = min_albedo;
    T.motion = rows.p; T.motionN = motion ? nrows : 0; T.histCap = hist_cap;
    const dim3 grid((unsigned)((P + kBlock - 1) / kBlock));
    PTCHECK(timed_launches(reps, ms, [&]() -> int {
        if (albedo) {
            if (form == 3) temporal_motion_launch<kTemporalFilterDemod, true>(motion != 0, grid, T);
            else if (form == 2) temporal_motion_launch<kTemporalMoments, true>(motion != 0, grid, T);
            else if (form == 1) temporal_motion_launch<kTemporalCapture, true>(motion != 0, grid, T);
            else temporal_motion_launch<kTemporalFilter, true>(motion != 0, grid, T);
        } else {
            if (form == 2) temporal_motion_launch<kTemporalMoments, false>(motion != 0, grid, T);
            else if (form == 1) temporal_motion_launch<kTemporalCapture, false>(motion != 0, grid, T);
            else temporal_motion_launch<kTemporalFilter, false>(motion != 0, grid, T);
        }
        return PT_OK;
    }));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(out4, out.p, P * sizeof(float4), hipMemcpyDeviceToHost));
    if (albedo) HIPCHECK(hipMemcpy(out_a4, outA.p, P * sizeof(float4), hipMemcpyDeviceToHost));
    if (needN) PTCHECK(download(out_n, outN, P));
    return PT_OK;
}

int pt_test_noise_stats(const float *rgb_sum, const float *lum_sq_sum, int w, int h, int samples, float threshold, float lum_floor, PtNoiseStats *out,
                        size_t stats_struct_bytes, float *tile_rel_var_host, int tiles_per_wave, int reps, float *ms) {
    NEED_GPU();
    if (!rgb_sum || !lum_sq_sum || !out || stats_struct_bytes != sizeof(PtNoiseStats) || w < 1 || h < 1 || samples < 2 || !noise_positive(threshold) ||
        !noise_positive(lum_floor) || (ms && reps < 1) || tiles_per_wave < 0 || tiles_per_wave > 64)
        return fail(PT_ERR_INVALID, "pt_test_noise_stats: bad argument");
    const size_t P = (size_t)w * h, tiles = (size_t)((w + kNoiseTile - 1) / kNoiseTile) * (size_t)((h + kNoiseTile - 1) / kNoiseTile);
    DevBuf<float> S, Q, map, var;
    DevBuf<uint32_t> frame;
    PTCHECK(S.upload(rgb_sum, P * 3));
    PTCHECK(Q.upload(lum_sq_sum, P));
    int rc = frame.alloc(2); if (rc) return rc;
    if (tile_rel_var_host) { rc = map.alloc(tiles); if (rc) return rc; }
    const float thr2 = threshold * threshold;
    const int tpw = tiles_per_wave ? tiles_per_wave : kNoiseTilesPerWave;
    uint32_t words[2] = {0u, 0u};
    rc = noise_launch(S.p, Q.p, w, h, samples, lum_floor, thr2, frame.p, map.p, nullptr, nullptr, tpw); if (rc) return rc;
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(words, frame.p, sizeof words, hipMemcpyDeviceToHost));
    if (tile_rel_var_host) PTCHECK(download(tile_rel_var_host, map, tiles));
    noise_fill(out, w, h, samples, thr2, words, 0.0f);
    if (!ms) return PT_OK;
    if (P > 0x7fffffffull - kBlock) return fail(PT_ERR_INVALID, "pt_test_noise_stats: k_variance indexes with an int");
    rc = var.alloc(P); if (rc) return rc;
    const int tilesX = (w + kNoiseTile - 1) / kNoiseTile;
    const dim3 gridN((unsigned)((tiles + 4 * tpw - 1) / (4 * tpw))), gridV((unsigned)((P + kBlock - 1) / kBlock));
    const float n = (float)samples, nM1 = (float)(samples - 1);
    Event ev[3];
    for (Event &e : ev) PTCHECK(e.create(hipEventDefault));
    hipLaunchKernelGGL(k_variance, gridV, dim3(kBlock), 0, nullptr, S.p, Q.p, (int)P, n, nM1, var.p);      // (k_noise_stats has run above)
    for (int r = 0; r < reps; ++r) {
        HIPCHECK(hipMemsetAsync(frame.p, 0, 2 * sizeof(uint32_t), nullptr));
        HIPCHECK(hipEventRecord(ev[0], nullptr));
        hipLaunchKernelGGL(k_noise_stats, gridN, dim3(kBlock), 0, nullptr, S.p, Q.p, w, h, tilesX, (int)tiles, tpw, n, nM1, lum_floor, thr2, frame.p, map.p);
        HIPCHECK(hipEventRecord(ev[1], nullptr));
        hipLaunchKernelGGL(k_variance, gridV, dim3(kBlock), 0, nullptr, S.p, Q.p, (int)P, n, nM1, var.p);
        HIPCHECK(hipEventRecord(ev[2], nullptr));
        HIPCHECK(hipEventSynchronize(ev[2]));
        HIPCHECK(hipEventElapsedTime(&ms[2 * r], ev[0], ev[1]));
        HIPCHECK(hipEventElapsedTime(&ms[2 * r + 1], ev[1], ev[2]));
    }
    HIPCHECK(hipGetLastError());
    return PT_OK;
}

int pt_test_sincos(const float *x, int n, float *s, float *c) {
    NEED_GPU();
    if (n <= 0) return PT_OK;
    DevBuf<float> a, ds, dc;
    PTCHECK(a.upload(x, n));
    PTCHECK(ds.alloc(n));
    PTCHECK(dc.alloc(n));
    PTCHECK(launch_wait(k_test_sincos, blocks_for(n), 0, a.p, n, ds.p, dc.p));
    PTCHECK(download(s, ds, n));
    return download(c, dc, n);
}

int pt_test_reflect_refract(const float *I3, const float *N3, const float *eta, int n, float *refl3, float *refr3) {
    NEED_GPU();
    if (n <= 0) return PT_OK;
    DevBuf<float> a, b, e, r1, r2;
    PTCHECK(a.upload(I3, (size_t)n * 3));
    PTCHECK(b.upload(N3, (size_t)n * 3));
    PTCHECK(e.upload(eta, n));
    PTCHECK(r1.alloc((size_t)n * 3));
    PTCHECK(r2.alloc((size_t)n * 3));
    PTCHECK(launch_wait(k_test_reflect_refract, blocks_for(n), 0, a.p, b.p, e.p, n, r1.p, r2.p));
    PTCHECK(download(refl3, r1, (size_t)n * 3));
    return download(refr3, r2, (size_t)n * 3);
}

int pt_test_texture_sample(const float *rgb, int w, int h, const float *uv2, int n, float *rgb_out3) {
    NEED_GPU();
    if (w < 1 || h < 1 || w > kTexSizeMax || h > kTexSizeMax || !rgb || n < 0 || (n && (!uv2 || !rgb_out3)))
        return fail(PT_ERR_INVALID, "pt_test_texture_sample: bad argument");
    if (n == 0) return PT_OK;
    std::vector<float4> tx((size_t)w * h);
    for (size_t q = 0; q < tx.size(); ++q) tx[q] = make_float4(rgb[3 * q], rgb[3 * q + 1], rgb[3 * q + 2], 0.0f);
    DevBuf<float4> t;
    DevBuf<float> a, o;
    PTCHECK(t.upload(tx));
    PTCHECK(a.upload(uv2, (size_t)n * 2));
    PTCHECK(o.alloc((size_t)n * 3));
    PTCHECK(launch_wait(k_test_texture_sample, blocks_for(n), 0, t.p, w, h, a.p, n, o.p));
    return download(rgb_out3, o, (size_t)n * 3);
}

int pt_test_texture_uv(int kind, const float *in, const int32_t *face, int n, float *uv_out2) {
    NEED_GPU();
    if (kind < 0 || kind > 2 || n < 0 || (n && (!in || !uv_out2 || (kind == 1 && !face)))) return fail(PT_ERR_INVALID, "pt_test_texture_uv: bad argument");
    if (n == 0) return PT_OK;
    if (kind == 1)
        for (int i = 0; i < n; ++i)
            if (face[i] < 0 || face[i] > 5) return fail(PT_ERR_INVALID, "pt_test_texture_uv: face %d", face[i]);
    DevBuf<float> a, o;
    DevBuf<int> f;
    PTCHECK(a.upload(in, (size_t)n * (kind == 2 ? 8 : 3)));
    if (kind == 1) PTCHECK(f.upload(face, n));
    PTCHECK(o.alloc((size_t)n * 2));
    PTCHECK(launch_wait(k_test_texture_uv, blocks_for(n), 0, kind, a.p, f.p, n, o.p));
    return download(uv_out2, o, (size_t)n * 2);
}

int pt_test_bump_normal(const float *height, int w, int h, const int32_t *kind, const float *in, int n, float *out) {
    NEED_GPU();
    if (w < 1 || h < 1 || w > kTexSizeMax || h > kTexSizeMax || !height || n < 0 || (n && (!kind || !in || !out)))
        return fail(PT_ERR_INVALID, "pt_test_bump_normal: bad argument");
    if (n == 0) return PT_OK;
    std::vector<float4> tx((size_t)w * h), tan(2 * (size_t)n, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (size_t q = 0; q < tx.size(); ++q) tx[q] = make_float4(height[q], height[q], height[q], 0.0f);
    for (int i = 0; i < n; ++i) {
        if (kind[i] < 0 || kind[i] > 2) return fail(PT_ERR_INVALID, "pt_test_bump_normal: kind %d", kind[i]);
        const float *e = in + 40 * (size_t)i;
        if (kind[i] == 1 && !(e[23] >= 0.0f && e[23] <= 5.0f && e[23] == (float)(int)e[23]))
            return fail(PT_ERR_INVALID, "pt_test_bump_normal: face %g", e[23]);
        if (kind[i] == 2) meshTangents(e + 28, e + 22, tan[2 * (size_t)i], tan[2 * (size_t)i + 1]);
    }
    DevBuf<float4> t, tg;
    DevBuf<float> a, o;
    DevBuf<int> k;
    PTCHECK(t.upload(tx));
    PTCHECK(tg.upload(tan));
    PTCHECK(a.upload(in, (size_t)n * 40));
    PTCHECK(k.upload(kind, n));
    PTCHECK(o.alloc((size_t)n * 16));
    PTCHECK(launch_wait(k_test_bump_normal, blocks_for(n), 0, t.p, w, h, k.p, a.p, tg.p, n, o.p));
    return download(out, o, (size_t)n * 16);
}
