/*
 * pt_amd_test.h -- TEST-ONLY entry points of the MI355X path-tracing hot path (libpt_amd_test.so).
 *
 * Not part of the drop-in boundary: the product library libpt_amd.so (include/pt_amd.h) exports none of these.  The same
 * single source (csrc/pt_api.hip) is linked a second time with -DPT_TEST_API into libpt_amd_test.so, which adds the entry
 * points below -- the __device__ functions of the render kernels evaluated one by one over host arrays (parity tests of
 * SURVEY 8 rows a6-a12, a19), the device-side soundness sweeps of every culling shortcut, and a hook that sets the
 * renderer's fault word by hand.  Only tests/ and profiles/ load that library.
 */
#ifndef PT_AMD_TEST_H
#define PT_AMD_TEST_H

#include "pt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- diagnostics of a renderer: the instance that lives in THIS library (initialise it with this library's pt_init) ----
 * State of the paths still alive after `bounces` bounces of iteration `iter`, sorted by pixel index (the device queue order is
 * arrival order): arrays of capacity W*H (x3).  Does not touch the accumulator.  (Rounds 1-4 exported it from the product.) */
int pt_debug_trace_paths(int iter, int bounces, float *origin3, float *dir3, float *color3,
                         int32_t *pixelIndex, int32_t *count);

/* ---- device primitives evaluated on the GPU over HOST arrays (parity tests of rows a6-a12, a19):
 * the same __device__ functions the render kernels call. ------------------------------------------ */
int pt_test_utilhash(const uint32_t *in, uint32_t *out, int n);
int pt_test_rng(const uint32_t *seeds, int nseeds, int ndraws, float *u01_out /* nseeds*ndraws */);
/* rays: n x 6; each ray against ONE geom (geoms[geom_index[i]]); outputs keep their input values
 * on a miss like the reference's out-parameters (intersections.h:86-88,114-126). */
int pt_test_intersect(const PtGeom *geoms, int ngeoms, const int32_t *geom_index, const float *rays,
                      int n, float *t, float *p3, float *n3, int32_t *outside);
/* sphereCertainMiss (world-space culling of spheres) soundness: `rays` pseudo-random rays against the spheres
 * of `geoms`; *violations = rays culled although the full test hits (must be 0), *culled = rays culled. */
int pt_test_sphere_cull_sweep(const PtGeom *geoms, int ngeoms, uint64_t seed, int64_t rays, uint64_t *culled,
                              uint64_t *violations);
/* sphereHalfLineExcess (pt_device.h: the certificate of the sphere-heavy sweep of the later bounces -- the squared distance of a sphere's
 * centre from the HALF-line, direction normalised approximately) swept like certainMiss: `rays` rays in three families (aimed near the
 * ball from 1/64 .. 64 units; leaving the sphere's own surface as a scatter does; from within 2 % of the bounding ball's surface),
 * directions unit and not.  *culled = certified misses, *behind = those with the centre behind the origin, *violations = certified
 * although src/intersections.h:101-143 returns a hit (must be 0). */
int pt_test_sphere_halfline_sweep(const PtGeom *geoms, int ngeoms, uint64_t seed, int64_t rays, uint64_t *culled, uint64_t *behind,
                                  uint64_t *violations);
/* The sphere CLUSTERS' box certificates (sphere-heavy scenes without meshes: a survivor's class bits 3 / 4 say which of the two clusters of
 * spheres its ray can hit; pt_api.hip: build_sphere_clusters builds them for `geoms` -- a whole scene, spheres and cubes -- exactly as
 * pt_init does) soundness: `rays` rays in four families (scatters off the spheres; from the scene's extent towards a cluster's box and
 * its shell; from close to a box; axis- and plane-parallel directions).  certified2[g] = certificates issued for cluster g, *violations
 * = spheres of a cluster certified as missed that src/intersections.h:101-143 hits (must be 0).  info18 (may be null): the bound on
 * the origins, the size of cluster 0 in the table, the two boxes {lo, hi, -, -}. */
int pt_test_sphere_cluster_sweep(const PtGeom *geoms, int ngeoms, uint64_t seed, int64_t rays, uint64_t *certified2, uint64_t *violations,
                                 float *info18);
/* ... and of the sphere GROUPS' bounding balls (k_bounce<..., GROUPS>: scenes of hundreds of swept primitives, pt_init: build_sphere_groups): a group
 * certified as missed sends the ray through the full test of each of its 16 members; a hit is a violation (must be 0) */
int pt_test_sphere_group_sweep(const PtGeom *geoms, int ngeoms, uint64_t seed, int64_t rays, uint64_t *certified, uint64_t *violations, int32_t *ngroups);
/* ... and the clusters themselves for inspection (host only, no GPU needed): info18 as above; table[k] = the primitive behind entry k of the
 * sweep's table (cluster 0 = entries 0 .. info18[1] - 1, padded to an even count with a copy of its last sphere; then cluster 1 -- whose end pt_init
 * pads likewise), *ntable entries (<= table_cap). */
int pt_test_sphere_clusters(const PtGeom *geoms, int ngeoms, float *info18, int32_t *table, int32_t table_cap, int32_t *ntable);
/* ... and the whole table of the swept primitives as pt_init would build it for a SCENE (host only, no GPU needed; pt_init's arguments as
 * pt_test_scene_plan takes them): the plan's own phases up to plan_swept, which calls build_sphere_clusters and build_sphere_groups -- so a
 * scene that a later phase refuses (plan_lds) still shows its table.  table[e] = the primitive behind entry e, padding included;
 * entries5[5 e ..] = entry e's {centre (3), threshold (scaled), K} as the device reads them; info6 = {entries (nSphCull), n0 (entries of
 * cluster 0, 0: no clusters), grpN0 (its groups), nSphGroups, swept primitives (0: the scene is not sphere-heavy), grouped (0 / 1)};
 * bounds2 = {grpOMax, sphDirScale}; balls4[4 g ..] = group g's ball as the device reads it, {centre (3), threshold}, nSphGroups of them.
 * A scene that is not grouped has no groups: entries in file order of its clusters, nSphGroups 0. */
int pt_test_sphere_groups(const PtCamera *cam, const PtGeom *geoms, int ngeoms, const PtMaterial *mats, int nmats, int traceDepth, const PtOptions *opts,
                          int32_t *table, float *entries5, int32_t table_cap, float *balls4, int32_t balls_cap, int32_t info6[6], float bounds2[2]);
/* wallCertainMiss (world-space culling of large cubes against their inflated bounding boxes, which classes the queue by
 * the wall a path can still hit) soundness: as above, for the cubes of `geoms`. */
int pt_test_wall_box_sweep(const PtGeom *geoms, int ngeoms, uint64_t seed, int64_t rays, uint64_t *culled,
                           uint64_t *violations);
/* The slab certificate's two evaluations on the caller's rays (rays: n x {origin3, direction3}) against ONE cube and its inflated world
 * box: flags[i] bit 0 = wallCertainMiss from three reciprocals formed once (k_bounce's PLAIN forms: shared with the walls' block), bit 1 =
 * wallCertainMissByAxis (the other forms), bit 2 = the origin's |x| + |y| + |z| lies within the box's bound, bit 3 = the full box test
 * hits.  box7 (or NULL) = the box {lo3, hi3} and the bound.  n = 0: the box alone. */
int pt_test_slab_decisions(const PtGeom *cube, const float *rays, int n, uint32_t *flags, float *box7);
/* wallPlanesPossible / wallPlanesOriented (the one-plane-per-wall certificates of the survivors' queue classes; pt_init's choose_walls numbers the cubes of
 * `geoms` as walls exactly as a render would) soundness: `rays` pseudo-random rays from the walls' inner faces, the corners, the
 * interior and beyond; *violations = (ray, wall) pairs certified as missed although the full test hits (must be 0), *certified =
 * certificates issued, *single = rays left with exactly one possible wall, *nplane = walls that have a plane. */
int pt_test_wall_plane_sweep(const PtGeom *geoms, int ngeoms, uint64_t seed, int64_t rays, int32_t *nplane, uint64_t *certified,
                             uint64_t *violations, uint64_t *single);
/* (host only, no GPU needed) the planes pt_init's choose_walls keeps for ROTATED walls (ptd::wallPlanesOriented, round 5): planes[w] =
 * {unit normal towards the scene's interior (3), threshold, far} of plane wall w, wall_geom[i] = the primitive that is wall i (walls with
 * an axis slot first, then the plane walls, then the rest), *nslot / *nplane / *nwalls their counts.  planes: 6 x 5 floats, wall_geom: 6 ints. */
int pt_test_wall_planes(const PtGeom *geoms, int ngeoms, float *planes, int32_t *wall_geom, int32_t *nslot, int32_t *nplane, int32_t *nwalls);
/* Screen-space culling of camera rays (per-primitive pixel rectangles, their union, the per-row primitive lists with their hull
 * spans -- everything pt_init derives from the camera, built here by the very same host functions) soundness: every pixel of
 * `cam`'s frame sends `samples` camera rays through the full tests of every primitive; *violations = hits from a pixel the culling
 * would have skipped (must be 0), *culled = (ray, primitive) pairs the culling skips, *hits = hits.  Spheres and cubes. */
int pt_test_camera_cull_sweep(const PtCamera *cam, const PtGeom *geoms, int ngeoms, int samples, uint64_t *hits, uint64_t *culled,
                              uint64_t *violations);
/* ... and the MARGIN of the tables' object-space inflation (pt_api.hip: inflated_object_box): for every hit of the same sweep, the
 * fraction of the inflation the hit needs -- 0 for a geometric hit, up to 1 for a hit the fp32 test's rounding created, above 1 for a
 * hit outside the inflated box -- evaluated in double precision on the exact object-space half-line.  *worst_fraction = the largest
 * (its reciprocal is the safety margin), *needed = hits with a fraction above 0.  Primitives whose culling is off are skipped. */
int pt_test_camera_cull_margin(const PtCamera *cam, const PtGeom *geoms, int ngeoms, int samples, double *worst_fraction, uint64_t *needed);
/* The same tables for inspection (host only, no GPU needed): rects4[4 i ..] = primitive i's pixel rectangle, scene_rect4 = their
 * union, spans2[2 (y ngeoms + i) ..] = the pixels x0 .. x1 of row y from which primitive i is reachable (x0 > x1: none). */
int pt_test_camera_cull_tables(const PtCamera *cam, const PtGeom *geoms, int ngeoms, int32_t *rects4, int32_t *scene_rect4, int32_t *spans2);
/* The camera rays' packed work list pt_init builds from those tables for shard (shard_rank, shard_count), here without its length cap
 * (host only, no GPU needed).  sizes4 = {lanes of the list (-1: not built), entries of sig_idx, pixels listed, pixels of the shard}.
 * pix[lane] = x | y << 16 or 0xffffffff (padding), wave2[2 w ..] = {first, end} of wave w's primitives in sig_idx.  Call with pix,
 * wave2 or sig_idx NULL for the sizes alone: pix takes sizes4[0] words, wave2 sizes4[0] / 32, sig_idx sizes4[1]. */
int pt_test_camera_list(const PtCamera *cam, const PtGeom *geoms, int ngeoms, int shard_rank, int shard_count, uint32_t *pix, int32_t *wave2,
                        int32_t *sig_idx, int64_t *sizes4);
/* The same list as pt_init builds it for the untextured forms: a one-cube signature's pixels split by the cube face every camera ray of
 * theirs is certified to enter through (pt_host_scene.h: camera_face_certificate), face[w] = 2 axis + (side > 0) for wave w, or -1
 * (host only).  sizes4 = {lanes (-1: not built), entries of sig_idx, pixels listed, pixels in resolved waves}; face takes sizes4[0] / 64. */
int pt_test_camera_resolved(const PtCamera *cam, const PtGeom *geoms, int ngeoms, int shard_rank, int shard_count, uint32_t *pix, int32_t *wave2,
                            int32_t *sig_idx, int32_t *face, int64_t *sizes4);
/* The same list with the certificates evaluated on the DEVICE between the list's two passes, as the camera move (pt_init with PT_SAME_SCENE) evaluates them
 * (csrc/pt_camera_faces.h: k_camera_faces): every array must equal pt_test_camera_resolved's.  kernel_ms (or NULL): the launches' time. */
int pt_test_camera_resolved_device(const PtCamera *cam, const PtGeom *geoms, int ngeoms, int shard_rank, int shard_count, uint32_t *pix, int32_t *wave2,
                                   int32_t *sig_idx, int32_t *face, int64_t *sizes4, float *kernel_ms);
/* Which way the calling thread's last camera move (pt_init with PT_SAME_SCENE) went: *fast = 1 (every buffer kept), 0 (pt_init inside), -1 before the first move and
 * after a refusal; the tables the fast path uploaded, and their bytes. */
int pt_test_last_camera_move(int *fast, int *tables_uploaded, int *bytes_uploaded);
/* A full pt_init call with PT_FLAG_KEEP_RENDERER reports through pt_test_last_camera_move as well: the move's figures where it matched the live renderer, the state
 * "before the first move" (-1, 0, 0) where it ran the full call.  pt_test_keep_mismatch: WHY the calling thread's last such call did not match -- the name of the
 * first comparison that failed ("geoms", "materials", "traceDepth", "flags", "max_batch", "texels", "texture UVs", "no live renderer", ...), "" where it matched. */
int pt_test_keep_mismatch(char *why, int bytes);
/* Device sweep: for every resolved pixel of the unsharded list, `samples` seeded jitters and the four corners of the certificate's
 * footprint -- the resolved wave's box test (pt_device.h: boxFaceHit) against boxIntersectionTest.  counts = {rays, rays on which
 * (t > 0, outside, face, P bit for bit) differ -- must be 0 --, resolved pixels}. */
int pt_test_face_hit_sweep(const PtCamera *cam, const PtGeom *geoms, int ngeoms, int samples, uint64_t seed, uint64_t counts[3]);
/* The later bounces' counterpart (pt_device.h: wallFaceCertificate, boxFacePoint; pt_host_scene.h: choose_wall_faces).
 * pt_test_wall_faces (host only): what pt_init would plan for the scene, per primitive -- face[i] = the inner face 2 axis + (side > 0) of a
 * wall that has one, else -1; beyond[i] = the least side * o_axis (object space) the certificate is issued from, else 0; ngeoms entries
 * each.  PT_AMD_NO_WALL_RESOLVE=1 (read by the plan, tests only): every face -1.
 * pt_test_wall_face_sweep: `geoms` = cubes, the walls of a room as pt_init chooses and numbers them; `rays` pseudo-random rays from the
 * room at the walls' inner faces -- dense at their edges and corners and in grazes, a few with NaN, inf and zero components.  counts =
 * {rays the certificate accepts; of those, rays on which boxFacePoint and boxIntersectionTest<true, false>(., false, true) differ in
 * (return value > 0, outside, face, P bit for bit) -- must be 0; rays it rejects although the box test hits from outside through the
 * face; rays it rejects in all}.
 * pt_test_wall_resolve_tally: the test library's own tally of its renderer's later bounces since the last call, per wave and tile --
 * {wave-tiles that hold a path; of them one-wall tiles whose wall has a face; of those the waves that took the face; lanes whose
 * certificate failed} -- read and cleared.  The product library keeps no such tally. */
int pt_test_wall_faces(const PtCamera *cam, const PtGeom *geoms, int ngeoms, const PtMaterial *mats, int nmats, int traceDepth, const PtOptions *opts,
                       int32_t *face, float *beyond);
int pt_test_wall_face_sweep(const PtGeom *geoms, int ngeoms, uint64_t seed, int64_t rays, uint64_t counts[4]);
int pt_test_wall_resolve_tally(uint64_t counts[4]);
/* pt_test_candidate_tally: the test library's tally of the later bounces' CANDIDATE tiles since the last call, read and cleared.  Per wave
 * and tile: {[0] later wave-tiles that hold a path; [1] of them candidate tiles (a class bit above the wall's three set: their list holds
 * binned primitives); [2] of those the tiles of ONE wall that has an inner face, in the forms that resolve one-wall tiles (the tiles a
 * certified face inside candidate tiles would serve: measured and not kept, profiles/candidate_tiles.txt); [3] lanes of
 * candidate tiles whose nearest hit is a binned primitive}.  Per scatter of a scene that bins: {[4] paths that live on; [5] of them the
 * candidates by the bounding balls alone; [6] the candidates by the rule in force -- the ball, and a second certificate by the primitive's
 * kind (KParams::binBox): for a cube the slab certificate ALONE, for a sphere the half-line ball; [7] the candidates by the ball beside
 * that rule (<= [6]: what evaluating a cube's ball as well would leave)}.  PT_AMD_NO_TIGHT_CANDIDATES=1 (read by the plan, tests only): no second
 * certificate, [7] = [6] = [5]. */
int pt_test_candidate_tally(uint64_t counts[8]);
/* pt_test_group_tally: the test library's tally of the GROUPED sweep of the later bounces (k_bounce<..., GROUPS>) since the last call, read
 * and cleared.  Per wave and tile: {[0] rounds of 64 groups run; [1] waves that ran level 2 from LDS; [2] waves that ran it from global
 * memory (more than kGroupLdsMax entries); [3] calls of passes() from inside the group loop: a lane's column of kCandPairs parked words was
 * full}.  Per lane: {[4] group words parked; [5] the largest number of words any lane had parked at once (a maximum)}.  A renderer that is
 * not grouped tallies nothing. */
int pt_test_group_tally(uint64_t counts[6]);
/* Triangle meshes.  pt_test_mesh_intersect: `n` rays against ONE mesh geom on the GPU, through the hierarchy (flat = 0) or a
 * plain list of its triangles (flat = 1: the brute-force rule); outputs keep their input values on a miss; culled[i] = 1 when
 * the bounding-ball test (certainMiss) rejected the ray -- t[i] is NaN if the full test hits nevertheless (must not happen).
 * pt_test_mesh_bvh (host only, no GPU needed): the records pt_init would build, in units of 4 words (pt_device.h: MeshUnit) --
 * the triangles in file order, three units each (v0, v1, v2, the mesh's box margin as floats, two words unused), one unit of
 * padding when that is an odd number of units, then the inner nodes of the copy laid out for rays of direction octant `octant`
 * (bit a set: the direction's component a is negative), two units each, nearer child first: six half-precision planes in three
 * words (entry x, y, z, exit x, y, z; entry = lo where the direction is positive, hi where negative; lo rounded down, hi up)
 * and the child's ref, then the same for the far child; refs in units relative to this array, bit 31 = a triangle;
 * *nrecs in = capacity in units, out = unit count; *stack_need = far children that can wait at once on a lane's stack, over
 * all eight copies. */
int pt_test_mesh_intersect(const PtGeom *geom, const float *tris, int ntris, int flat, const float *rays, int n, float *t,
                           float *p3, float *n3, int32_t *outside, int32_t *culled);
int pt_test_mesh_bvh(const float *tris, int ntris, int octant, uint32_t *units4, int *nrecs, int *stack_need);
/* pt_test_mesh_intersect with the mesh's attributes and the WINNER's name: `normals` (9 floats per triangle: vertex normals, or NULL: flat
 * shading) and `mats` (one scene material per triangle, -1 = the object's, or NULL) as PtMesh's; the same outputs, plus tri[i] = the file
 * index of the triangle that was hit (-1 on a miss) and face_mat[i] = that triangle's own material (-1: it has none, or a miss).  The
 * index is read off a second walk of the same rays through the same records with word 10 of triangle k set to 1 + k: the walk itself
 * (ptd::meshIntersectionTest) is the render kernels', unchanged. */
int pt_test_mesh_intersect2(const PtGeom *geom, const float *tris, const float *normals, const int32_t *mats, int ntris, int flat,
                            const float *rays, int n, float *t, float *p3, float *n3, int32_t *outside, int32_t *culled, int32_t *tri,
                            int32_t *face_mat);
/* certainMiss soundness for a mesh geom: `rays` pseudo-random rays dense in grazes of its bounding ball (origins 1/64 .. 64
 * radii away); *violations = rays the bounding-ball test rejected although the walk hits (must be 0), *hits = rays that hit */
int pt_test_mesh_cull_sweep(const PtGeom *geom, const float *tris, int ntris, uint64_t seed, int64_t rays, uint64_t *culled,
                            uint64_t *violations, uint64_t *hits);
/* slabQuotients (shared-reciprocal packed division of the box test) next to the compiler's correctly
 * rounded `/`: per-element outputs, and a device-side pseudo-random sweep that returns the number of
 * bit mismatches over `pairs` (o, d) pairs (must be 0). */
int pt_test_slab_quotients(const float *o, const float *d, int n, float *t1, float *t2, float *ref1, float *ref2);
int pt_test_slab_quotients_sweep(uint64_t seed, int64_t pairs, uint64_t *mismatches);
/* The box test's fast slab phase (pt_device.h: boxSlabsFast -- comparisons on approximate quotients wherever their outcome is beyond
 * doubt, ONE exact quotient, the reference's loop as the fallback) against the reference's loop alone: `rays` pseudo-random rays per
 * call against the cubes of `geoms`, dense in edges, corners, grazes, surface origins, degenerate directions.  counts[0] = rays,
 * [1] = rays the fast path decided, [2] = hits among those, [3] = bit mismatches of (t, P, normal source, outside) -- must be 0.
 * div_mismatches[0]: the fast normalize's reciprocal against 1.0f / s on every float of [2^-40, 2^40]; [1]: the one exact quotient
 * against a / d on 2^30 pairs of the box test's range -- both must be 0. */
int pt_test_box_fast_sweep(const PtGeom *geoms, int ngeoms, uint64_t seed, int64_t rays, uint64_t counts[4], uint64_t div_mismatches[2]);
/* sqrtUnscaled (the correctly rounded sqrt without its exponent-range handling, used by the hemisphere sampler)
 * next to the compiler's sqrt on every fp32 bit pattern of its range (+-0 and [2^-96, inf)), and inverseSqrtNearOne
 * (the re-normalisation of getPointOnRay) next to 1.0f / sqrtf on every bit pattern: mismatches[0] and [2] must be 0,
 * [1] = patterns inside sqrtUnscaled's range, [3] = patterns on inverseSqrtNearOne's short path (513). */
int pt_test_unscaled_sqrt_sweep(uint64_t mismatches[4]);
/* sets the renderer's device fault word by hand (2; 0 clears it in every slot), so that the reporting path can be tested */
int pt_test_force_fault(int which);
/* the next `count` assemblies of the group issue their ncclReduce with a NULL communicator (ncclInvalidArgument): the error path of
 * pt_group_reduce / pt_group_iterate / pt_group_readback -- ncclGroupEnd must still run and a later call must succeed */
int pt_test_group_fail_next_reduce(PtGroup *g, int count);
/* a group whose member i sits on VIRTUAL device vdev[i] (0 <= vdev[i] < 8, vdev[0] == 0: the root), every one of them on the current HIP device.
 * Each distinct virtual device is a GroupDevice of its own -- its own full-frame accumulator, snapshot pair, collective stream and events --
 * exactly as a distinct HIP device would be; everything downstream (pt_group_init / iterate / reduce / readback / sync / counters / destroy,
 * pt_test_group_fail_next_reduce) is the product's code, unchanged.  collective 0: host gather; 1: the emulated reduce below.
 * pt_group_collective() answers "host gather" or "emulated reduce (virtual devices: test library)". */
int pt_test_group_create_virtual(PtGroup **out, int n, const int32_t *vdev, int collective);
/* The emulated reduce (csrc/pt_group.h: EmulatedReduce -- ncclReduce's semantics in one process: at the end of a call group the root's
 * recvbuf[i] = sendbuf_0[i] + sendbuf_1[i] + ... in ascending rank order, fp32, in place allowed, by ONE kernel on the root's stream behind an
 * event of every other rank's stream) on its own: send_host[r] = rank r's `count` floats, 1..8 ranks, root 0; in_place 1: the root receives into
 * its own send buffer.  recv_host = what the root received; send_after_host (or NULL; entries may be NULL) = every rank's device send buffer as
 * the call left it -- the other ranks' unchanged, the root's too unless in place. */
int pt_test_emulated_reduce(const float *const *send_host, int ranks, int64_t count, int in_place, float *recv_host, float *const *send_after_host);
int pt_test_hemisphere(const float *normals3, const int32_t *iter_index_depth3, int n, float *out3);
int pt_test_sincos(const float *x, int n, float *s, float *c);
int pt_test_pow(const float *x, const float *e, int n, float *out);   /* build-defined x^e of the imperfect-specular sampler */
int pt_test_reflect_refract(const float *I3, const float *N3, const float *eta, int n, float *refl3,
                            float *refr3);
/* texture mapping (pt_amd.h, pt_device.h "texture mapping"): the kernels' own device functions over host arrays.
 * pt_test_texture_sample: one texture of w x h texels (rgb: w * h * 3 floats, row 0 = top) at n coordinate pairs uv2 -> rgb_out3.
 * pt_test_texture_uv: n texture coordinates -> uv_out2.  kind 0 (sphere): in = n x 3, the object-space hit point; kind 1 (cube): the same,
 * face[i] = the hit face (axis * 2 + (sign > 0)); kind 2 (mesh): in = n x 8, {u, v} the barycentrics and the triangle's corner UVs
 * {u0, v0, u1, v1, u2, v2}.  `face` is read for cubes only (may be NULL otherwise). */
int pt_test_texture_sample(const float *rgb, int w, int h, const float *uv2, int n, float *rgb_out3);
int pt_test_texture_uv(int kind, const float *in, const int32_t *face, int n, float *uv_out2);
/* bump mapping (pt_amd.h, pt_device.h "bump mapping"): the kernels' gradient, tangents and shading normal over host arrays.  One height map of
 * w x h texels (row 0 = top); per hit kind[i] (0 sphere, 1 cube, 2 mesh) and 40 floats of `in`: {scale, outside (0 / 1), N (3), dir (3),
 * transform (12, column-major 3 x 4)}, then sphere: the object-space hit point q; cube: q and the face (axis * 2 + (sign > 0), as a float);
 * mesh: the barycentric u, v, the corner UVs u0 v0 u1 v1 u2 v2 and the object-space corners p0 p1 p2 (tangents: the library's own host code).
 * out: 16 floats per hit {hu, hv, Pu (3), Pv (3), Ns (3), bumped (0 / 1), u, v, 0, 0}; Ns = N where the hit stays unbumped. */
int pt_test_bump_normal(const float *height, int w, int h, const int32_t *kind, const float *in, int n, float *out);
/* the denoiser (pt_amd.h, csrc/pt_denoise.h): pt_denoise of THIS library's renderer with the form of k_atrous_*<AtrousPlain> named -- 0: the product's
 * choice per level, 1: the plain gather, 2 / 3: LDS tiles of 64 x 4 / 64 x 8 pixels of a residue class -- every form gives the same bits.
 * ms (or NULL): 1 + levels kernel times by HIP events, k_gbuffer first (0 when the guide buffers were cached), then each level. */
int pt_test_denoise(int samples, const PtDenoiseParams *p, size_t params_struct_bytes, int form, float *rgb_mean_host, float *ms);
/* ... and pt_denoise_var with the form of k_atrous_*<AtrousGuided> named, the same four forms; var_host may be NULL; ms as above (on a renderer whose context
 * holds history -- PT_FLAG_TEMPORAL -- k_temporal runs between k_gbuffer and level 0 and belongs to neither time; so do the two launches of the
 * spatial variance estimate for samples 1, which only a PT_FLAG_SPATIAL_VARIANCE renderer accepts). */
int pt_test_denoise_var(int samples, const PtDenoiseVarParams *p, size_t params_struct_bytes, int form, float *rgb_mean_host, float *var_host, float *ms);
/* the display path (PT_FLAG_DISPLAY_FILTER, pt_amd.h) of THIS library's renderer -- any PT_FLAG_MOMENTS renderer, the flag itself is not needed
 * -- with the form of k_atrous_*<AtrousGuided> named for every level, the last included: what pt_iterate(..., rgba8_dev) enqueues behind the commit, into
 * rgba8_dev (DEVICE memory, W * H * 4 bytes), on the renderer's stream, without a synchronisation unless ms is given.  form: the four of
 * pt_test_denoise.  fused 1: the last level writes the bytes itself (k_atrous_*<AtrousGuided, false, true, ., true>); 0: it writes packed RGB and
 * k_to_rgba8 converts it -- the same bytes.  samples 1: the plain conversion -- on a PT_FLAG_SPATIAL_VARIANCE renderer the filter, as for
 * every other count.  ms (or NULL): 1 + PT_DISPLAY_LEVELS kernel times as pt_test_denoise_var's, the last level's with the k_to_rgba8 launch
 * where fused is 0 (all 0 for the plain conversion). */
int pt_test_display(int samples, int form, int fused, void *rgba8_dev, float *ms);
int pt_test_exp_neg_poly(const float *a, int n, float *out);   /* the filter's range weight, ptd::expNegPoly */
/* temporal reprojection (pt_amd.h, csrc/pt_temporal.h).  cam16 = the old view's camera as k_temporal takes it, 16 floats: eye (3), pixLenX,
 * pixLenY, halfW, halfH, then the rows r0, r1, r2 of the inverse of [view | -right | -up].
 * pt_test_temporal_camera (host only, no GPU needed): cam16 of a PtCamera, by the function pt_init's capture calls.
 * pt_test_temporal: k_temporal over host arrays of any w x h, no renderer needed -- capture 0: the filter form, out4 = (c, variance), out_n unused
 * (may be NULL); capture 1: out4 = Hc', out_n = Hn'; capture 2: the moments form, out4 = M, out_n = N (uncapped).  The current view: rgb_sum = S (w * h * 3), lum_sq_sum = Q (w * h), pos_t4 / nrm_id4 its guide
 * buffers as the device holds them (w * h * 4 each, .w of the second = the bits of the int32 primitive index); the history: hc4, hn, hpos_t4,
 * hnrm_id4 likewise.  ms (or NULL) with reps >= 1: `reps` kernel times by HIP events, after one untimed launch.
 * pt_test_history: the history THIS library's current context holds -- wh2 = its frame size, {0, 0}: none (nothing else is written then); every
 * other pointer may be NULL. */
int pt_test_temporal_camera(const PtCamera *cam, float *cam16);
int pt_test_temporal(int capture, int w, int h, int samples, const float *rgb_sum, const float *lum_sq_sum, const float *pos_t4, const float *nrm_id4,
                     const float *hc4, const float *hn, const float *hpos_t4, const float *hnrm_id4, const float *cam16, float *out4, float *out_n,
                     int reps, float *ms);
int pt_test_history(int32_t *wh2, float *hc4, float *hn, float *hpos_t4, float *hnrm_id4, float *cam16);
/* the spatial variance estimate (pt_amd.h, csrc/pt_spatial_var.h): k_spatial_variance_*<radius> over host arrays of any w x h, no renderer
 * needed.  radius 1, 2 or 3 (the product holds PT_SPATIAL_RADIUS only); form 0: the plain gather, 1: the LDS tiles -- both give the same bits.
 * m4 = M (w * h * 4: mean r, g, b, m2), n = N (w * h), pos_t4 / nrm_id4 the guide buffers as the device holds them; sigma_normal, sigma_position
 * > 0 as pt_denoise_var takes them (+inf: term off).  out4 = (c, variance), w * h * 4.  ms (or NULL) with reps >= 1: `reps` kernel times by HIP
 * events, after one untimed launch. */
int pt_test_spatial_variance(int radius, int form, int w, int h, const float *m4, const float *n, const float *pos_t4, const float *nrm_id4,
                             float sigma_normal, float sigma_position, float *out4, int reps, float *ms);
/* albedo demodulation (pt_amd.h, csrc/pt_albedo.h).
 * pt_test_albedo: the albedo sums of THIS library's renderer (PT_FLAG_DEMODULATE) behind everything enqueued, W * H * 4 floats: .xyz the sum of
 * the committed iterations' first-hit albedo, .w their number.  Synchronises.
 * pt_test_demodulate: k_demodulate and the levels behind it over host arrays of any w x h, no renderer needed: `levels` levels of the
 * variance-guided filter, level 0 as a later level at step 1, the last one AtrousDemod's, every level in the form named (1: the plain gather,
 * 2 / 3: LDS tiles of 64 x 4 / 64 x 8 pixels -- every form gives the same bits).  asum4 = the albedo sums (w * h * 4), samples >= 1 the count
 * they are divided by, min_albedo the floor.  inplace 0: k_demodulate reads the accumulators rgb_sum (w * h * 3) and lum_sq_sum (w * h),
 * samples >= 2, img4 unused; inplace 1: it rewrites img4 (w * h * 4: r, g, b, variance), the accumulators unused.  pos_t4 / nrm_id4: the guide buffers as the device holds
 * them; the sigmas as pt_denoise_var takes them.  demod4_out (or NULL): k_demodulate's image.  bytes 0: rgb_out (w * h * 3) and var_out (or
 * NULL) receive the last level's packed RGB and variance; bytes 1: rgba_out (w * h * 4 bytes) receives its BYTES form's, rgb_out / var_out
 * unused.  ms (or NULL) with reps >= 1: 2 * reps kernel times by HIP events, {k_demodulate, the last level} alternating, after one untimed
 * run (a timed inplace run demodulates an image again and again: its results are void). */
int pt_test_albedo(float *asum4_host);
int pt_test_demodulate(int form, int inplace, int bytes, int w, int h, int samples, int levels, const float *rgb_sum, const float *lum_sq_sum, const float *img4,
                       const float *asum4, const float *pos_t4, const float *nrm_id4, float sigma_lum, float sigma_normal, float sigma_position,
                       float min_albedo, float *demod4_out, float *rgb_out, float *var_out, uint8_t *rgba_out, int reps, float *ms);
/* demodulated history (pt_amd.h, csrc/pt_temporal.h under "ALBEDO").
 * pt_test_temporal_albedo: the ALBEDO forms of k_temporal over host arrays of any w x h, no renderer needed.  form 0 / 1 / 2: the filter, the
 * capture and the moments form as pt_test_temporal's `capture` names them; out4 / out_n as there.  asum4 = the current view's albedo sums
 * (w * h * 4), ha4 = the history's albedo (w * h * 4; .w is not read), the rest as pt_test_temporal takes it; out_a4 receives (Ab, tot).
 * front (form 0 alone, else 0): 0 the blend as it is; 1 the FUSED front, k_temporal<kTemporalFilterDemod, true>, one launch; 2 the two
 * launches it fuses, k_temporal<kTemporalFilter, true> and k_demodulate<true> in place with (asum = Ab, samples = 1) -- 1 and 2 give the same
 * bits; min_albedo is their floor.  ms (or NULL) with reps >= 1: `reps` times of the whole front by HIP events, after one untimed run.
 * pt_test_history_albedo: the albedo image of the history THIS library's current context holds -- wh2 = its frame size, {0, 0}: no history,
 * or one made by a renderer without PT_FLAG_DEMOD_HISTORY (nothing else is written then); ha4 (w * h * 4, or NULL): (Ab, tot). */
int pt_test_temporal_albedo(int form, int front, int w, int h, int samples, const float *rgb_sum, const float *lum_sq_sum, const float *pos_t4,
                            const float *nrm_id4, const float *asum4, const float *hc4, const float *hn, const float *ha4, const float *hpos_t4,
                            const float *hnrm_id4, const float *cam16, float min_albedo, float *out4, float *out_n, float *out_a4, int reps, float *ms);
int pt_test_history_albedo(int32_t *wh2, float *ha4);
/* object history (pt_amd.h, csrc/pt_temporal.h under "MOTION").  A motion table is `nrows` rows of 24 floats (ptk::MotionRow): m[3][4] row by
 * row, then (G[0][0..2], the bits of the int32 state), (G[1][0..2], 0), (G[2][0..2], 0).
 * pt_test_motion_table (host only, no GPU needed): the table pt_init makes between the geoms a history's view was rendered with (`then`) and
 * a call's (`now`), ngeoms rows, by the function pt_init calls; *any = 1 where a row has another state than 0 (pt_init keeps a table then).
 * pt_test_history_motion: the table of the history THIS library's current context holds, as the device holds it -- *nrows = 0: none (no
 * history, or every primitive unmoved); rows24 (or NULL) receives nrows * 24 floats, cap (or NULL) the count's cap the blends take.
 * pt_test_temporal_motion: any (FORM, ALBEDO, MOTION) form of k_temporal over host arrays of any w x h, no renderer needed.  form 0 / 1 / 2 as
 * pt_test_temporal's `capture`, 3: kTemporalFilterDemod (albedo 1 alone).  albedo 0: asum4, ha4 and out_a4 are not read (NULL allowed);
 * motion 0: rows24, nrows and hist_cap are not read.  hist_cap: step 6's cap.  Everything else as pt_test_temporal_albedo takes it. */
int pt_test_motion_table(const PtGeom *then, const PtGeom *now, int ngeoms, float *rows24, int32_t *any);
int pt_test_history_motion(int32_t *nrows, float *rows24, float *cap);
int pt_test_temporal_motion(int form, int albedo, int motion, int w, int h, int samples, const float *rgb_sum, const float *lum_sq_sum,
                            const float *pos_t4, const float *nrm_id4, const float *asum4, const float *hc4, const float *hn, const float *ha4,
                            const float *hpos_t4, const float *hnrm_id4, const float *cam16, const float *rows24, int nrows, float hist_cap,
                            float min_albedo, float *out4, float *out_n, float *out_a4, int reps, float *ms);
/* the noise statistics (pt_amd.h, csrc/pt_noise.h): k_noise_stats -- the kernel pt_noise_stats launches -- over host arrays of any w x h, no
 * renderer needed: rgb_sum = S (w * h * 3), lum_sq_sum = Q (w * h); out, tile_rel_var_host (or NULL) as pt_noise_stats.  tiles_per_wave: how many
 * tiles a wave of the grid takes, 1..64, 0 = the library's choice -- every value gives the same bits.  ms (or NULL) with
 * reps >= 1: 2 * reps kernel times by HIP events, {k_noise_stats, k_variance over the same arrays} alternating, after one untimed launch of each. */
int pt_test_noise_stats(const float *rgb_sum, const float *lum_sq_sum, int w, int h, int samples, float threshold, float lum_floor, PtNoiseStats *out,
                        size_t stats_struct_bytes, float *tile_rel_var_host, int tiles_per_wave, int reps, float *ms);
/* The selector of k_bounce's forms (host only, no GPU needed): state_bits = a renderer's state and a launch's `first` -- bit 0 first, 1 dof
 * (thin lens), 2 many, 3 sweptCubes, 4 mesh, 5 grouped, 6 tex, 7 bump, 8 plain -- -> *form_bits = the nine template flags of the
 * instantiation the launch takes (bit 0 FIRST, 1 MANY, 2 DOF, 3 MESH, 4 PLAIN, 5 CUBES, 6 GROUPS, 7 TEX, 8 BUMP), by the very function
 * pt_init calls; PT_ERR_INVALID when the library holds no such instantiation (a state no renderer reaches). */
int pt_test_bounce_form(uint32_t state_bits, uint32_t *form_bits);
/* The state pt_init left in THIS library's renderer (host only): *state_bits = its dof, many, sweptCubes, mesh, grouped, tex, bump and plain
 * in the bit order pt_test_bounce_form takes them, bit 0 (`first`, a launch's) clear; PT_ERR_NOT_INIT before pt_init. */
int pt_test_renderer_state(uint32_t *state_bits);
/* What pt_init would plan for a scene, without a device (host only; csrc/pt_scene_plan.h: plan_scene): pt_init's arguments, with the meshes,
 * textures and bindings registered with THIS library.  PT_OK and a summary of the plan -- state_bits as pt_test_renderer_state gives them --
 * or the refusal pt_init would answer with (PT_ERR_INVALID, pt_last_error); no renderer is touched either way. */
typedef struct PtTestPlanSummary {
    uint32_t state_bits;
    int32_t nBinned, nWalls, nSphCull, nSphGroups, nLocalPad, firstSkipped, poolChunks;
    uint64_t ldsBytes, ldsBytesNext;
    int32_t histBits;       /* 0: the path pools carry a path's throughput (44 B); b > 0: its material history in codes of b bits (32 B: the PLAIN forms) */
    int32_t grpLds;         /* grouped scenes: 1 = the later bounces stage the table's level-2 data in LDS, 0 = they read it from global memory (else 0) */
} PtTestPlanSummary;
int pt_test_scene_plan(const PtCamera *cam, const PtGeom *geoms, int ngeoms, const PtMaterial *mats, int nmats, int traceDepth, const PtOptions *opts,
                       PtTestPlanSummary *out);
/* device allocations THIS library's renderers and temporaries hold right now (every one has one owner type, which counts in this
 * library only): 0 after pt_free */
int64_t pt_test_live_device_buffers(void);
/* ... and the streams plus events plus page-locked host allocations they, its groups and the scan library hold (the same: one owner type
 * each, counted in this library only): 0 after pt_free and pt_group_destroy */
int64_t pt_test_live_handles(void);
/* The scene tables pt_init allocated for THIS library's renderer (host only, from the plans): out[0] the poses it holds (1, or
 * PT_MOTION_STEPS under PT_FLAG_MOTION), out[1] / out[2] the device buffers and bytes of ONE pose's own tables (step 0's), out[3] / out[4] of
 * the tables held once whatever the number of poses (texels, mesh records), out[5] the bytes of every pose's own tables together: the
 * renderer's scene tables are out[4] + out[5] bytes in out[3] + out[0] x out[1] buffers.  PT_ERR_NOT_INIT before pt_init. */
int pt_test_pose_tables(int64_t out[6]);

#ifdef __cplusplus
}
#endif
#endif /* PT_AMD_TEST_H */
