// pt_host_scene.h -- host side of pt_init: what the kernels need to know about a scene, derived once per pt_init in double precision or with
// the very fp32 operations the kernels would issue -- packed primitives and materials (GeomDev, MaterialDev), the walls' inflated boxes and
// one-plane certificates, the sphere clusters of sphere-heavy scenes, the camera constants and the screen-space culling tables of the
// camera-ray bounce.  Pure host code: no renderer state, no HIP call.  Header-only part of the single translation unit pt_api.hip
// (inside its anonymous namespace).
#pragma once

// `box`: the object-space bounds lo[3], hi[3] of the primitive -- nullptr = the unit cube [-0.5, 0.5]^3 of a sphere or cube,
// a mesh passes the union of its (inflated) triangle boxes.
void pack_geom(const PtGeom &g, GeomDev &d, const float *eye = nullptr, const float *box = nullptr) {
    memset(&d, 0, sizeof d);
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 3; ++r) {
            d.inv[c * 3 + r] = g.inverseTransform[c * 4 + r];
            d.xf[c * 3 + r] = g.transform[c * 4 + r];
            d.invT[c * 3 + r] = g.invTranspose[c * 4 + r];
        }
    for (int r = 0; r < 3; ++r) d.invZ[r] = d.inv[9 + r] * 0.0f;
    d.type = g.type == PT_CUBE ? 1 : 0;                   // (a mesh's normal is made like a sphere's: type 0, flags bit 5)
    d.flags = d.cullFlags = g.type == PT_CUBE ? 1 : (g.type == PT_MESH ? 32 : 0);    // bit 1 (binned) is set by pt_init
    d.meshRoot = ptd::kMeshEnd;                           // set by pt_init / the mesh tests
    d.material = g.materialid;
    // bounding-ball culling data (ptd::certainMiss): bounds smax >= sigma_max, smin <= sigma_min of the 3x3 part
    double A[3][3], Ai[3][3];
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) { A[c][r] = g.transform[c * 4 + r]; Ai[c][r] = g.inverseTransform[c * 4 + r]; }
    double len[3], fro = 0, froi = 0;
    bool orth = true;
    for (int c = 0; c < 3; ++c) {
        len[c] = std::sqrt(A[c][0] * A[c][0] + A[c][1] * A[c][1] + A[c][2] * A[c][2]);
        for (int r = 0; r < 3; ++r) { fro += A[c][r] * A[c][r]; froi += Ai[c][r] * Ai[c][r]; }
    }
    for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 3; ++b) {
            const double dp = A[a][0] * A[b][0] + A[a][1] * A[b][1] + A[a][2] * A[b][2];
            if (!(std::fabs(dp) <= 1e-5 * len[a] * len[b])) orth = false;
        }
    double smax, smin;
    if (orth) {            // rotation x scale: the singular values are the column lengths
        smax = std::max(len[0], std::max(len[1], len[2])) * (1 + 1e-5);
        smin = std::min(len[0], std::min(len[1], len[2])) * (1 - 1e-5);
    } else {               // any matrix: Frobenius bounds
        smax = std::sqrt(fro);
        smin = froi > 0 ? 1.0 / std::sqrt(froi) : 0.0;
    }
    d.centre[0] = g.transform[12]; d.centre[1] = g.transform[13]; d.centre[2] = g.transform[14];
    double rho2 = g.type == PT_SPHERE ? 0.25 : 0.75;       // object-space bounding ball: the sphere / the cube's corners
    bool boxOk = true;
    if (box) {
        // a mesh: the ball around the centre of its box.  The margins of certainMiss are relative to the ball; they cover the
        // rounding of the object-space evaluation (relative to the distance from the object-space ORIGIN) only while the
        // mesh is not far off its own origin: otherwise it is never culled.
        double c[3], far = 0;
        rho2 = 0;
        for (int a = 0; a < 3; ++a) {
            c[a] = 0.5 * ((double)box[a] + box[3 + a]);
            const double h = 0.5 * ((double)box[3 + a] - box[a]);
            rho2 += h * h;
            far = std::max(far, std::max(std::fabs((double)box[a]), std::fabs((double)box[3 + a])));
        }
        rho2 *= 1 + 1e-6;                                  // (the centre is rounded to float below)
        for (int r = 0; r < 3; ++r)
            d.centre[r] = (float)((double)g.transform[0 + r] * c[0] + (double)g.transform[4 + r] * c[1] + (double)g.transform[8 + r] * c[2] +
                                  (double)g.transform[12 + r]);
        boxOk = std::isfinite(rho2) && rho2 > 0 && far <= 100.0 * std::sqrt(rho2);
    }
    const double r2 = rho2 * smax * smax * (1 + 1e-3), kk = smin > 0 ? 1e-4 * (smax / smin) * (smax / smin) : INFINITY;
    const bool ok = boxOk && std::isfinite(r2) && std::isfinite(kk) && kk < 0.5 && smin > 0;
    d.boundR = (float)(std::sqrt(rho2) * smax);
    d.cullR2 = ok ? (float)r2 : INFINITY;      // infinite radius: never culled
    d.cullK = ok ? (float)kk : 0.0f;
    d.rect[0] = d.rect[1] = 0;                 // whole frame until pt_init projects the primitive (project_geom)
    d.rect[2] = d.rect[3] = 0x7fffffff;
    if (g.type == PT_CUBE) {
        // Per face: ptd::normalize(ptd::mulMV(xf, +-e_axis, 0)) and ptd::hemisphereFrame of that normal, operation by
        // operation (this file is built with -ffp-contract=off; host sqrt and division are correctly rounded like the
        // device's): what cubeFrameVector() looks up.
        struct V { float x, y, z; };
        auto normalize = [](V a) {
            const float xx = a.x * a.x, yy = a.y * a.y, zz = a.z * a.z;
            const float xy = xx + yy;
            const float dt = xy + zz;                                 // glm dot: (x*x + y*y) + z*z
            const float inv = 1.0f / std::sqrt(dt);                   // glm::inversesqrt
            return V{a.x * inv, a.y * inv, a.z * inv};
        };
        auto cross = [](V x, V y) {                                   // glm/detail/func_geometric.inl:134-143
            const float a0 = x.y * y.z, a1 = y.y * x.z, b0 = x.z * y.x, b1 = y.z * x.x, c0 = x.x * y.y, c1 = y.x * x.y;
            return V{a0 - a1, b0 - b1, c0 - c1};
        };
        const float kSqrtOneThird = 0.5773502691896257645091487805019574556476f;   // src/utilities.h:15
        const float *m = d.xf;
        for (int axis = 0; axis < 3; ++axis)
            for (int pos = 0; pos < 2; ++pos) {
                float v[3] = {0.0f, 0.0f, 0.0f};
                v[axis] = pos ? 1.0f : -1.0f;
                float r[3];
                for (int c = 0; c < 3; ++c) {
                    const float a0 = m[0 + c] * v[0], a1 = m[3 + c] * v[1], a2 = m[6 + c] * v[2], a3 = m[9 + c] * 0.0f;
                    const float s01 = a0 + a1, s23 = a2 + a3;
                    r[c] = s01 + s23;
                }
                const V n = normalize(V{r[0], r[1], r[2]});
                V notNormal;
                if (std::fabs(n.x) < kSqrtOneThird) notNormal = V{1, 0, 0};
                else if (std::fabs(n.y) < kSqrtOneThird) notNormal = V{0, 1, 0};
                else notNormal = V{0, 0, 1};
                const V p1 = normalize(cross(n, notNormal));
                const V p2 = normalize(cross(n, p1));
                float *out = d.cubeFrame + 9 * (2 * axis + pos);
                out[0] = n.x; out[1] = n.y; out[2] = n.z;
                out[3] = p1.x; out[4] = p1.y; out[5] = p1.z;
                out[6] = p2.x; out[7] = p2.y; out[8] = p2.z;
            }
    }
    if (eye) {   // ptd::mulMV(inv, eye, 1) in the same operation order (this file is built with -ffp-contract=off)
        const float *m = d.inv;
        for (int r = 0; r < 3; ++r) {
            const float a0 = m[0 + r] * eye[0], a1 = m[3 + r] * eye[1], a2 = m[6 + r] * eye[2], a3 = m[9 + r] * 1.0f;
            const float s01 = a0 + a1, s23 = a2 + a3;
            d.camObj[r] = s01 + s23;
        }
    }
}
// World-space box of a cube, INFLATED for ptd::wallCertainMiss: the 8 corners of the unit cube through `transform` in double
// precision, widened by delta = 4e-5 S, S = max(diagonal of the box, largest |coordinate|), and rounded outwards to float.
// Why 4e-5: a scattered ray starts 1e-3 off the surface it leaves (spec S6), and the certificate has to be able to tell
// that it leaves -- delta must stay below that offset for a scene of Cornell's size (S = 14: delta = 5.7e-4) -- while the
// reference's own evaluation moves the boundary by ~2e-7 (|o| + S) (object-space transform, thin axis: products of
// magnitude 100 |o| rounded to 2^-24, scaled back by 1/100), i.e. 1.2e-5 for |o| + S <= 60 = *omax: a margin of 47x.
// Returns S (a negative value when the cube is not finite); *omax receives the largest |x| + |y| + |z| of a ray origin
// for which that margin holds, 5 S - (largest |coordinate|).
double wall_box(const PtGeom &g, WallBox &w, double *omax = nullptr) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int corner = 0; corner < 8; ++corner) {
        const double o[3] = {(corner & 1) ? 0.5 : -0.5, (corner & 2) ? 0.5 : -0.5, (corner & 4) ? 0.5 : -0.5};
        for (int r = 0; r < 3; ++r) {
            const double q = (double)g.transform[0 + r] * o[0] + (double)g.transform[4 + r] * o[1] + (double)g.transform[8 + r] * o[2] +
                             (double)g.transform[12 + r];
            if (!std::isfinite(q)) return -1.0;
            lo[r] = std::min(lo[r], q);
            hi[r] = std::max(hi[r], q);
        }
    }
    double diag = 0, big = 0;
    for (int r = 0; r < 3; ++r) {
        diag += (hi[r] - lo[r]) * (hi[r] - lo[r]);
        big = std::max(big, std::max(std::fabs(lo[r]), std::fabs(hi[r])));
    }
    const double S_ = std::max(std::sqrt(diag), big);
    const double delta = 4e-5 * S_;
    if (omax) *omax = 5.0 * S_ - big;
    memset(&w, 0, sizeof w);
    w.face = -1;                            // (no inner face: choose_wall_faces names one)
    for (int r = 0; r < 3; ++r) {
        w.lo[r] = std::nextafter((float)(lo[r] - delta), -INFINITY);
        w.hi[r] = std::nextafter((float)(hi[r] + delta), INFINITY);
        if (!std::isfinite(w.lo[r]) || !std::isfinite(w.hi[r])) return -1.0;
    }
    return S_;
}

// Sphere-heavy scenes: the spheres in TWO SPATIAL CLUSTERS.  `sc` (every sphere's packed culling data, thresholds already scaled) is split at
// the median centre along one axis and reordered, cluster 0 first (n0 entries, even: padded with a copy of its last one).  A survivor's class bits
// 3 / 4 say which clusters its ray can hit (k_bounce: a slab certificate, ptd::wallCertainMiss, against each cluster's box), and a tile of the
// next bounce sweeps only those.  The binned primitives (group 0) share bit 3: axis and order of the halves are the ones with the smallest sum of
// (surface area of what a bit stands for) x (spheres behind it).  A choice that only steers which tiles skip which tests; results never depend on it.
// What the certificate rests on: box g holds, for every sphere of cluster g, the ball of radius sqrt(cullR2 + K ocMax^2) (1 + 1e-6) around its
// centre -- the sphere's own half-line certificate (ptd::sphereHalfLineExcess: distance^2 of the centre from the half-line > cullR2 + K |oc|^2, with
// |oc| <= ocMax = omax + |centre| for every origin a certificate is issued for, |x| + |y| + |z| <= omax) holds for every half-line that misses
// that ball -- and is inflated like a wall's box (wall_box: delta = 4e-5 S against ~2e-7 (|o| + S) of rounding in the slab test, |o| <= 5 S).
// Returns false (and leaves everything as it was) when no clusters can be built: fewer than two spheres, or one that is never culled.
// (tests/test_gpu_parity.py::test_sphere_cluster_boxes_never_reject_a_hit: pt_test_sphere_cluster_sweep, 2^28 rays, 0 violations.)
bool build_sphere_clusters(const PtGeom *geoms, int ngeoms, const std::vector<GeomDev> &hg, const std::vector<int> &binned, std::vector<SphereCull> &sc,
                           int &n0, float &omaxOut, float box[2][8]) {
    // a sphere's half-line ball for the origins certificates are issued for: radius^2 = cullR2 + K ocMax^2 (scaled thresholds: the larger)
    auto build = [&](const std::vector<SphereCull> &v, double omax, double lo[3], double hi[3]) {
        for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
        for (const SphereCull &e : v) {
            const double cn = std::sqrt((double)e.centre[0] * e.centre[0] + (double)e.centre[1] * e.centre[1] + (double)e.centre[2] * e.centre[2]);
            const double ocMax = omax + cn;
            const double r = std::sqrt((double)e.cullR2 + (double)e.cullK * ocMax * ocMax) * (1.0 + 1e-6);
            for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], (double)e.centre[a] - r); hi[a] = std::max(hi[a], (double)e.centre[a] + r); }
        }
    };
    auto area = [](const double lo[3], const double hi[3]) {
        const double x = hi[0] - lo[0], y = hi[1] - lo[1], z = hi[2] - lo[2];
        return x * y + y * z + z * x;
    };
    bool finite = true;
    for (const SphereCull &e : sc) finite = finite && std::isfinite(e.cullR2) && std::isfinite(e.cullK);
    if (!finite || sc.size() < 2) return false;
    double bestCost = INFINITY;
    std::vector<SphereCull> best0, best1;
    for (int axis = 0; axis < 3; ++axis)
        for (int swap = 0; swap < 2; ++swap) {
            std::vector<SphereCull> v = sc;
            std::stable_sort(v.begin(), v.end(), [&](const SphereCull &a, const SphereCull &b) { return a.centre[axis] < b.centre[axis]; });
            const size_t h = v.size() / 2;
            std::vector<SphereCull> c0(v.begin(), v.begin() + h), c1(v.begin() + h, v.end());
            if (swap) std::swap(c0, c1);
            double lo0[3], hi0[3], lo1[3], hi1[3];
            build(c0, 0.0, lo0, hi0);
            build(c1, 0.0, lo1, hi1);
            for (int i : binned) {                                // bit 3 also stands for the binned primitives
                const GeomDev &G = hg[i];
                for (int a = 0; a < 3; ++a) { lo0[a] = std::min(lo0[a], (double)G.centre[a] - G.boundR); hi0[a] = std::max(hi0[a], (double)G.centre[a] + G.boundR); }
            }
            const double cost = area(lo0, hi0) * (double)c0.size() + area(lo1, hi1) * (double)c1.size();
            if (cost < bestCost) { bestCost = cost; best0 = c0; best1 = c1; }
        }
    // (a scattered ray starts on a primitive: the scene's own extent, |x| + |y| + |z| over its bounding box, with a quarter to spare,
    // bounds the origins worth a certificate -- and K |oc|^2 grows with the bound)
    double omax = 0.0, S_[2], big_[2];
    {
        double slo[3] = {INFINITY, INFINITY, INFINITY}, shi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int i = 0; i < ngeoms; ++i) {
            WallBox wb;
            if (geoms[i].type == PT_CUBE && wall_box(geoms[i], wb) >= 0)
                for (int a = 0; a < 3; ++a) { slo[a] = std::min(slo[a], (double)wb.lo[a]); shi[a] = std::max(shi[a], (double)wb.hi[a]); }
            else if (std::isfinite(hg[i].boundR))
                for (int a = 0; a < 3; ++a) { slo[a] = std::min(slo[a], (double)hg[i].centre[a] - hg[i].boundR); shi[a] = std::max(shi[a], (double)hg[i].centre[a] + hg[i].boundR); }
        }
        for (int a = 0; a < 3; ++a) omax += std::max(std::fabs(slo[a]), std::fabs(shi[a]));
        omax *= 1.25;
        if (!std::isfinite(omax)) omax = 0.0;
    }
    float bx[2][8];
    for (int g = 0; g < 2; ++g) for (int q = 0; q < 8; ++q) bx[g][q] = 0.0f;
    for (int pass = 0; pass < 2; ++pass)          // pass 0: the boxes' sizes with |oc| = |c|, for the bound; pass 1: the boxes for the bound that gave
        for (int g = 0; g < 2; ++g) {
            double lo[3], hi[3];
            build(g ? best1 : best0, pass ? omax : 0.0, lo, hi);
            double diag = 0, big = 0;
            for (int a = 0; a < 3; ++a) {
                diag += (hi[a] - lo[a]) * (hi[a] - lo[a]);
                big = std::max(big, std::max(std::fabs(lo[a]), std::fabs(hi[a])));
            }
            S_[g] = std::max(std::sqrt(diag), big); big_[g] = big;
            if (!pass) omax = std::min(omax, 5.0 * S_[g] - big);
            else {
                const double delta = 4e-5 * S_[g];
                for (int a = 0; a < 3; ++a) {
                    bx[g][a] = std::nextafter((float)(lo[a] - delta), -INFINITY);
                    bx[g][3 + a] = std::nextafter((float)(hi[a] + delta), INFINITY);
                    finite = finite && std::isfinite(bx[g][a]) && std::isfinite(bx[g][3 + a]);
                }
                // (the boxes only grew since pass 0 -- and a box built for a larger bound than the final one is the conservative side)
                omax = std::min(omax, 5.0 * S_[g] - big_[g]);
            }
        }
    if (!finite || !(omax > 0.0) || !std::isfinite(omax)) return false;
    if (best0.size() % 2) best0.push_back(best0.back());      // (two per scalar load; testing a sphere twice changes nothing)
    sc = best0;
    sc.insert(sc.end(), best1.begin(), best1.end());
    n0 = (int)best0.size();
    omaxOut = std::nextafter((float)omax, 0.0f);
    memcpy(box, bx, sizeof bx);
    return true;
}

// Scenes of HUNDREDS of swept primitives (k_bounce<..., GROUPS>): the packed table in spatial GROUPS of kSphGroupSize consecutive entries, each
// with a bounding ball.  `sc` comes in as build_sphere_clusters left it (cluster 0 = [0, n0), cluster 1 = the rest; n0 = 0: no clusters) and
// leaves with every cluster's entries ordered by recursive median splits of their centres (the widest axis; the left side a multiple of the
// group size, so only a cluster's last group is short: padded with copies of its last entry -- testing a primitive twice changes nothing),
// cluster 0 padded to an EVEN number of groups; `groups` receives one entry per group in the table's own format (geom = -1).
// What a group's certificate rests on: its ball holds, for every member i, the ball of radius r_i = sqrt(cullR2_i + K_i ocMax_i^2) (1 + 1e-6)
// around the member's centre -- exactly the balls build_sphere_clusters' boxes hold --, ocMax_i = omax + |centre_i| for the origins with
// |x| + |y| + |z| <= omax.  The device tests the group like a member (ptd::sphereHalfLineExcessScaled, the scene's one scaled direction):
// x = |oc|^2 - s^2 p^2 > T = R^2 s^2 (1 + 1e-6) implies d^2 - K_max |oc|^2 >= x / s^2 > R^2 up to fp32 rounding of x (4 ulp of |oc|^2 = 2.4e-7
// |oc|^2, against K_max >= 1e-4), i.e. the exact half-line passes the group's ball at a distance -- and so every member's ball: each member's
// own certificate would hold, with the room its ball was given.  Origins beyond omax take every group (k_bounce).
// (tests/test_gpu_parity.py::test_sphere_group_balls_never_reject_a_hit: pt_test_sphere_group_sweep.)
void build_sphere_groups(std::vector<SphereCull> &sc, int &n0, double omax, float sdir, std::vector<SphereCull> &groups, int &grpN0) {
    const int S = kSphGroupSize;
    auto order = [&](std::vector<SphereCull> &v) {
        struct Rec {
            std::vector<SphereCull> &v;
            int S;
            void run(int lo, int hi) {
                if (hi - lo <= S) return;
                double cmin[3] = {INFINITY, INFINITY, INFINITY}, cmax[3] = {-INFINITY, -INFINITY, -INFINITY};
                for (int i = lo; i < hi; ++i)
                    for (int a = 0; a < 3; ++a) { cmin[a] = std::min(cmin[a], (double)v[(size_t)i].centre[a]); cmax[a] = std::max(cmax[a], (double)v[(size_t)i].centre[a]); }
                int axis = 0;
                for (int a = 1; a < 3; ++a)
                    if (cmax[a] - cmin[a] > cmax[axis] - cmin[axis]) axis = a;
                int mid = lo + ((hi - lo) / 2 + S - 1) / S * S;
                if (mid >= hi) mid = lo + (hi - lo) / 2 / S * S;
                if (mid <= lo) return;
                std::nth_element(v.begin() + lo, v.begin() + mid, v.begin() + hi, [axis](const SphereCull &x, const SphereCull &y) {
                    return x.centre[axis] < y.centre[axis] || (x.centre[axis] == y.centre[axis] && x.geom < y.geom);
                });
                run(lo, mid);
                run(mid, hi);
            }
        } r{v, S};
        r.run(0, (int)v.size());
        while (v.size() % (size_t)S) v.push_back(v.back());
    };
    std::vector<SphereCull> c0(sc.begin(), sc.begin() + n0), c1(sc.begin() + n0, sc.end());
    if (!c0.empty()) {
        order(c0);
        if ((c0.size() / (size_t)S) % 2) {      // an even number of groups: the last one once more (a copy first: insert() takes no range of its own vector)
            const std::vector<SphereCull> last(c0.end() - S, c0.end());
            c0.insert(c0.end(), last.begin(), last.end());
        }
    }
    if (!c1.empty()) order(c1);
    sc = c0;
    sc.insert(sc.end(), c1.begin(), c1.end());
    n0 = (int)c0.size();
    grpN0 = n0 / S;
    groups.clear();
    for (size_t g = 0; g * (size_t)S < sc.size(); ++g) {
        double c[3] = {0, 0, 0};
        for (int i = 0; i < S; ++i)
            for (int a = 0; a < 3; ++a) c[a] += (double)sc[g * S + i].centre[a] / S;
        SphereCull e;
        memset(&e, 0, sizeof e);
        for (int a = 0; a < 3; ++a) e.centre[a] = (float)c[a];
        double R = 0;
        for (int i = 0; i < S; ++i) {
            const SphereCull &m = sc[g * S + i];
            const double cn = std::sqrt((double)m.centre[0] * m.centre[0] + (double)m.centre[1] * m.centre[1] + (double)m.centre[2] * m.centre[2]);
            const double ocMax = omax + cn;
            const double r = std::sqrt((double)m.cullR2 + (double)m.cullK * ocMax * ocMax) * (1.0 + 1e-6);
            const double dx = (double)m.centre[0] - e.centre[0], dy = (double)m.centre[1] - e.centre[1], dz = (double)m.centre[2] - e.centre[2];
            R = std::max(R, std::sqrt(dx * dx + dy * dy + dz * dz) + r);
        }
        R *= 1.0 + 1e-6;
        e.cullR2 = std::nextafter((float)(R * R * (double)sdir * (double)sdir * (1.0 + 1e-6)), INFINITY);
        e.cullK = 0.0f;
        e.geom = -1;
        groups.push_back(e);
    }
    if (groups.size() % 2) groups.push_back(groups.back());      // (the table is read two entries per scalar load; the pad is never evaluated)
}

// the bound on the ray origins worth a certificate: a scattered ray starts on a primitive -- the scene's own extent, |x| + |y| + |z| over its
// bounding box, with a quarter to spare (as build_sphere_clusters takes it)
double scene_origin_bound(const PtGeom *geoms, int ngeoms, const std::vector<GeomDev> &hg) {
    double omax = 0.0, slo[3] = {INFINITY, INFINITY, INFINITY}, shi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = 0; i < ngeoms; ++i) {
        WallBox wb;
        if (geoms[i].type == PT_CUBE && wall_box(geoms[i], wb) >= 0)
            for (int a = 0; a < 3; ++a) { slo[a] = std::min(slo[a], (double)wb.lo[a]); shi[a] = std::max(shi[a], (double)wb.hi[a]); }
        else if (std::isfinite(hg[i].boundR))
            for (int a = 0; a < 3; ++a) { slo[a] = std::min(slo[a], (double)hg[i].centre[a] - hg[i].boundR); shi[a] = std::max(shi[a], (double)hg[i].centre[a] + hg[i].boundR); }
    }
    for (int a = 0; a < 3; ++a) omax += std::max(std::fabs(slo[a]), std::fabs(shi[a]));
    omax *= 1.25;
    return std::isfinite(omax) ? omax : 0.0;
}

// The walls of a scene -- its large cubes: not binned, finite, at most kWallMax of them, the largest first -- with what the survivors'
// certificates need (k_bounce: which wall can a scattered ray still hit?): the inflated world boxes (wall_box), the bound on the ray
// origins the margins hold for, and for the walls that have one the PLANE of their box that faces the scene's interior
// (ptd::wallPlanesPossible): with C the centre of the box `outer` around all the walls' boxes, a face of a wall's box whose whole box
// lies beyond C on that axis.  Six slots (axis x side) hold one wall each: a wall takes the free slot in which it lies farthest out
// (in units of the scene's extent), the largest walls choose first; walls without a slot (a box across the middle of the scene, a
// second wall on the same side) are numbered behind the others and keep the slab test.
// Thresholds: the plane moved towards the interior by slack = 2e-6 (wallOMax + |diagonal of outer|), five times the rounding of the
// ray's exit point.  A choice that only steers which tiles skip which tests; results never depend on it.
// wallGeom[w] = the primitive that is wall w.
void choose_walls(const PtGeom *geoms, int ngeoms, const std::vector<GeomDev> &hg, KParams &k, std::vector<WallBox> &hw, std::vector<int> &wallGeom) {
    std::vector<std::pair<double, int>> cand;
    for (int i = 0; i < ngeoms; ++i)
        if (geoms[i].type == PT_CUBE && !hg[i].binned) cand.emplace_back(-(double)hg[i].boundR, i);
    std::sort(cand.begin(), cand.end());
    std::vector<WallBox> boxes;
    std::vector<int> which;
    double omaxAll = INFINITY;
    for (size_t c = 0; c < cand.size() && (int)boxes.size() < kWallMax; ++c) {
        WallBox wb;
        double om = 0;
        if (wall_box(geoms[cand[c].second], wb, &om) < 0) continue;
        omaxAll = std::min(omaxAll, om);
        boxes.push_back(wb);
        which.push_back(cand[c].second);
    }
    const int n = (int)boxes.size();
    k.nWalls = n;
    k.wallOMax = n > 0 ? (float)omaxAll : 0.0f;      // the margin must hold for every wall
    k.nSlotWalls = 0;
    k.nPlaneWalls = 0;
    memset(k.planeN, 0, sizeof k.planeN);
    for (int sl = 0; sl < 6; ++sl) { k.slotTh[sl] = 0.0f; k.slotBit[sl] = 0u; }
    for (int a = 0; a < 3; ++a) k.outerLo[a] = k.outerHi[a] = 0.0f;
    wallGeom.clear();
    if (n == 0) return;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (const WallBox &b : boxes)
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], (double)b.lo[a]); hi[a] = std::max(hi[a], (double)b.hi[a]); }
    double diag = 0;
    for (int a = 0; a < 3; ++a) diag += (hi[a] - lo[a]) * (hi[a] - lo[a]);
    diag = std::sqrt(diag);
    const double slack = 2e-6 * (omaxAll + diag);
    // slot of every wall: 2 axis + (high side), or -1
    std::vector<int> slot(n, -1);
    std::vector<double> th(n, 0.0);
    bool taken[6] = {false, false, false, false, false, false};
    // ROTATED walls (an edge of the cube that is not parallel to a world axis): their world boxes are far larger than they are, so they
    // take no slot; the plane of the face that looks at C, the middle of `outer`, certifies them instead (ptd::wallPlanesOriented):
    // n = that face's unit normal towards C, th = the largest n . corner + the box's inflation (wall_box: 4e-5 S) + the slack (the
    // exit point's rounding as above, the two dot products', and n's own rounding to float: 3e-6 (wallOMax + |diagonal of outer|)).
    std::vector<int> rotated(n, 0);
    std::vector<std::array<double, 4>> plane(n);
    std::vector<double> planeS(n, 0.0);
    double Smax = 0;            // the largest inflation scale among the walls (wall_box)
    std::vector<std::array<double, 3>> allCorners;   // every wall's cube, corner by corner
    for (int w = 0; w < n; ++w) {
        const PtGeom &g = geoms[which[w]];
        WallBox tmp;
        Smax = std::max(Smax, wall_box(g, tmp));
        for (int q = 0; q < 8; ++q) {
            const double o[3] = {(q & 1) ? 0.5 : -0.5, (q & 2) ? 0.5 : -0.5, (q & 4) ? 0.5 : -0.5};
            std::array<double, 3> c;
            for (int r = 0; r < 3; ++r)
                c[r] = (double)g.transform[0 + r] * o[0] + (double)g.transform[4 + r] * o[1] + (double)g.transform[8 + r] * o[2] + (double)g.transform[12 + r];
            allCorners.push_back(c);
        }
    }
    const bool noOriented = getenv("PT_AMD_NO_ORIENTED_WALLS") && atoi(getenv("PT_AMD_NO_ORIENTED_WALLS"));     // (experiments: round 4's behaviour)
    for (int w = 0; w < n && std::isfinite(slack) && !noOriented; ++w) {
        const PtGeom &g = geoms[which[w]];
        bool aligned = true;
        for (int c = 0; c < 3; ++c) {           // column c of the transform: the world direction of the cube's edge c
            double m = 0;
            int big = 0;
            for (int r = 0; r < 3; ++r) m = std::max(m, std::fabs((double)g.transform[4 * c + r]));
            for (int r = 0; r < 3; ++r) big += std::fabs((double)g.transform[4 * c + r]) > 1e-7 * m ? 1 : 0;
            aligned = aligned && big <= 1;
        }
        if (aligned) continue;
        // (a SMALL rotated cube -- a tilted light under the ceiling -- keeps the slab test against its world box: the plane of one face says
        // little about a box that spans a fraction of the room, the box around it a lot)
        if ((double)hg[which[w]].boundR < 0.2 * diag) { rotated[w] = -1; continue; }
        double corner[8][3];
        for (int q = 0; q < 8; ++q) {
            const double o[3] = {(q & 1) ? 0.5 : -0.5, (q & 2) ? 0.5 : -0.5, (q & 4) ? 0.5 : -0.5};
            for (int r = 0; r < 3; ++r)
                corner[q][r] = (double)g.transform[0 + r] * o[0] + (double)g.transform[4 + r] * o[1] + (double)g.transform[8 + r] * o[2] + (double)g.transform[12 + r];
        }
        WallBox tmp;
        const double Sw = wall_box(g, tmp);
        const double C[3] = {0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])};
        double bestGap = 1e-3 * diag;           // (C clearly on the far side of the face, or no plane)
        for (int a = 0; a < 3; ++a)
            for (int sgn = -1; sgn <= 1; sgn += 2) {
                // outward normal of the face (sgn e_a in the cube's space): sgn x row a of the inverse transform; towards C: its negative
                double nn[3] = {-sgn * (double)g.inverseTransform[0 + a], -sgn * (double)g.inverseTransform[4 + a], -sgn * (double)g.inverseTransform[8 + a]};
                const double len = std::sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
                if (!(len > 0) || !std::isfinite(len)) continue;
                for (double &v : nn) v /= len;
                double th = -INFINITY;
                for (int q = 0; q < 8; ++q) th = std::max(th, nn[0] * corner[q][0] + nn[1] * corner[q][1] + nn[2] * corner[q][2]);
                const double gap = (nn[0] * C[0] + nn[1] * C[1] + nn[2] * C[2]) - th;
                if (gap > bestGap && std::isfinite(th)) {
                    bestGap = gap;
                    rotated[w] = 1;
                    plane[w] = {nn[0], nn[1], nn[2], th + 4e-5 * Sw + 3e-6 * (omaxAll + diag)};
                    planeS[w] = Sw;
                }
            }
        if (!rotated[w]) rotated[w] = -1;       // (rotated, no usable face: the slab test)
    }
    for (int w = 0; w < n && std::isfinite(slack); ++w) {            // (largest walls first)
        if (rotated[w] != 0) continue;
        double best = 0;
        for (int a = 0; a < 3; ++a) {
            const double C = 0.5 * (lo[a] + hi[a]), ext = std::max(hi[a] - lo[a], 1e-30);
            const double gLow = (C - boxes[w].hi[a]) / ext, gHigh = (boxes[w].lo[a] - C) / ext;
            if (gLow > best && !taken[2 * a] && std::isfinite((double)boxes[w].hi[a] + slack)) { best = gLow; slot[w] = 2 * a; th[w] = (double)boxes[w].hi[a] + slack; }
            if (gHigh > best && !taken[2 * a + 1] && std::isfinite((double)boxes[w].lo[a] - slack)) { best = gHigh; slot[w] = 2 * a + 1; th[w] = (double)boxes[w].lo[a] - slack; }
        }
        if (slot[w] >= 0) taken[slot[w]] = true;
    }
    for (int pass = 0; pass < 3; ++pass)                              // walls with a slot first, then those with a plane of their own, then the rest
        for (int w = 0; w < n; ++w)
            if ((slot[w] >= 0 ? 0 : (rotated[w] == 1 ? 1 : 2)) == pass) {
                const int idx = (int)wallGeom.size();
                hw[idx] = boxes[w];
                if (pass == 1) {
                    float *pn = k.planeN[k.nPlaneWalls++];
                    for (int q = 0; q < 3; ++q) pn[q] = (float)plane[w][q];
                    const float t = (float)plane[w][3];
                    pn[3] = (double)t < plane[w][3] ? std::nextafter(t, INFINITY) : t;          // (towards the interior: the certificate may only get rarer)
                    // `far`: the half-space n . x >= far holds every wall's inflated cube (the segment's end may only move OUTWARDS)
                    double farD = INFINITY;
                    for (const auto &c : allCorners) farD = std::min(farD, (double)pn[0] * c[0] + (double)pn[1] * c[1] + (double)pn[2] * c[2]);
                    farD -= 4e-5 * Smax + 3e-6 * (omaxAll + diag);
                    const float ff = (float)farD;
                    pn[4] = (double)ff > farD ? std::nextafter(ff, -INFINITY) : ff;
                }
                if (slot[w] >= 0) {
                    // rounded towards the interior: a threshold may only make the certificate rarer
                    const float t = (float)th[w];
                    k.slotTh[slot[w]] = (slot[w] & 1) ? ((double)t > th[w] ? std::nextafter(t, -INFINITY) : t) : ((double)t < th[w] ? std::nextafter(t, INFINITY) : t);
                    k.slotBit[slot[w]] = 1u << idx;
                    k.nSlotWalls = idx + 1;
                }
                wallGeom.push_back(which[w]);
            }
    for (int a = 0; a < 3; ++a) {       // rounded outwards
        k.outerLo[a] = std::nextafter((float)lo[a], -INFINITY);
        k.outerHi[a] = std::nextafter((float)hi[a], INFINITY);
    }
}

// The INNER FACE of every wall, for the later bounces' face certificate (ptd::wallFaceCertificate, where the argument is written out): the
// face of the wall's cube that looks at the middle C of `outer` -- the one a ray from the room enters the wall through --, as
// 2 K + (s > 0), and `beyond`, the least s o_K (object space) from which the certificate is issued.  Which face is named decides nothing
// about results: the certificate tests every ray against the face it is given.  What the host owes it is `beyond`, which keeps the hit's
// distance positive in the kernel's float32:
//     beyond = 1/2 + 2e-4 + 2^-18 (1 + wallOMax + |translation|_1 + |transform|_F) / smin(transform).
// The hit point lies tmin - 1e-4 >= beyond - 1/2 - 1e-4 object units along the unit object-space direction from the origin, i.e. at least
// smin (beyond - 1/2 - 1e-4) world units away, while the three transforms between the world origin and the world hit point -- origin to
// object space, the point along the ray, the point back to the world: sums of four products of magnitude at most |o|_1 + |translation|_1
// and 1.5 |transform|_F + |translation|_1, origins within wallOMax -- move them by less than 2^-20 (1 + wallOMax + |translation|_1 +
// |transform|_F) together: a quarter of the room that is left.  smin >= |det| / |transform|_F^2.
// A wall whose data cannot be bounded that way (a non-finite entry, a singular transform), or none of whose faces clearly looks at C,
// gets -1: its tiles run the box test.  `off` (PT_AMD_NO_WALL_RESOLVE, tests only): every wall -1.
void choose_wall_faces(const PtGeom *geoms, const KParams &k, const std::vector<int> &wallGeom, bool off, std::vector<WallBox> &hw) {
    for (WallBox &b : hw) { b.face = -1; b.beyond = 0.0f; }
    if (off) return;
    double C[3], diag = 0;
    for (int a = 0; a < 3; ++a) {
        C[a] = 0.5 * ((double)k.outerLo[a] + (double)k.outerHi[a]);
        diag += ((double)k.outerHi[a] - (double)k.outerLo[a]) * ((double)k.outerHi[a] - (double)k.outerLo[a]);
    }
    diag = std::sqrt(diag);
    if (!std::isfinite(diag)) return;
    for (size_t w = 0; w < wallGeom.size() && w < hw.size(); ++w) {
        const PtGeom &g = geoms[wallGeom[w]];
        double T2 = 0, l1t = 0;
        for (int r = 0; r < 3; ++r) {
            l1t += std::fabs((double)g.transform[12 + r]);
            for (int j = 0; j < 3; ++j) T2 += (double)g.transform[j * 4 + r] * (double)g.transform[j * 4 + r];
        }
        const double detT = (double)g.transform[0] * ((double)g.transform[5] * g.transform[10] - (double)g.transform[9] * g.transform[6]) -
                            (double)g.transform[4] * ((double)g.transform[1] * g.transform[10] - (double)g.transform[9] * g.transform[2]) +
                            (double)g.transform[8] * ((double)g.transform[1] * g.transform[6] - (double)g.transform[5] * g.transform[2]);
        if (!std::isfinite(T2) || !std::isfinite(detT) || !std::isfinite(l1t) || !(T2 > 0) || !(std::fabs(detT) > 0)) continue;
        const double smin = std::fabs(detT) / T2;
        const double beyond = 0.5 + 2e-4 + 0x1p-18 * (1.0 + (double)k.wallOMax + l1t + std::sqrt(T2)) / smin;
        if (!std::isfinite(beyond) || !(beyond <= 0x1p+18)) continue;
        double corner[8][3];
        bool fin = true;
        for (int q = 0; q < 8; ++q) {
            const double o[3] = {(q & 1) ? 0.5 : -0.5, (q & 2) ? 0.5 : -0.5, (q & 4) ? 0.5 : -0.5};
            for (int r = 0; r < 3; ++r) {
                corner[q][r] = (double)g.transform[0 + r] * o[0] + (double)g.transform[4 + r] * o[1] + (double)g.transform[8 + r] * o[2] + (double)g.transform[12 + r];
                fin = fin && std::isfinite(corner[q][r]);
            }
        }
        if (!fin) continue;
        double bestGap = 1e-3 * diag;           // (C clearly on the far side of the face, or no face)
        int best = -1;
        for (int a = 0; a < 3; ++a)
            for (int sgn = -1; sgn <= 1; sgn += 2) {
                // the outward normal of face (a, sgn): sgn x row a of the inverse transform -- C must lie beyond every corner along it
                double nn[3] = {sgn * (double)g.inverseTransform[0 + a], sgn * (double)g.inverseTransform[4 + a], sgn * (double)g.inverseTransform[8 + a]};
                const double len = std::sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
                if (!(len > 0) || !std::isfinite(len)) continue;
                for (double &v : nn) v /= len;
                double th = -INFINITY;
                for (int q = 0; q < 8; ++q) th = std::max(th, nn[0] * corner[q][0] + nn[1] * corner[q][1] + nn[2] * corner[q][2]);
                const double gap = (nn[0] * C[0] + nn[1] * C[1] + nn[2] * C[2]) - th;
                if (gap > bestGap && std::isfinite(th)) { bestGap = gap; best = 2 * a + (sgn > 0 ? 1 : 0); }
            }
        if (best < 0) continue;
        const float bf = (float)beyond;
        hw[w].face = best;
        hw[w].beyond = (double)bf < beyond ? std::nextafter(bf, INFINITY) : bf;      // (upwards: the certificate may only get rarer)
    }
}

// n / d for every n < 2^30 as (n * magic) >> shift: with s = ceil(log2 d), shift = 30 + s and magic = ceil(2^shift / d)
// (< 2^31) the error e = magic * d - 2^shift is below d <= 2^s, so n * e < 2^(30 + s) = 2^shift and the quotient is exact
// (Granlund-Montgomery); n * magic < 2^61 fits the 64-bit product.  (The camera-ray bounce divides path indices up to
// pixels x max_batch <= 2^29 by the shard's pixel count; rounds 1-2 used shift = 28 + s, exact only below 2^28.)
void magic_divisor(uint32_t d, uint32_t &magic, uint32_t &shift) {
    if (d <= 1) { magic = 1; shift = 0; return; }
    uint32_t s = 0;
    while ((1ull << s) < d) ++s;
    shift = 30 + s;
    magic = (uint32_t)(((1ull << shift) + d - 1) / d);
}

void pack_material(const PtMaterial &m, MaterialDev &d) {
    memset(&d, 0, sizeof d);
    d.color[0] = m.color.x; d.color[1] = m.color.y; d.color[2] = m.color.z;
    d.specColor[0] = m.specularColor.x; d.specColor[1] = m.specularColor.y; d.specColor[2] = m.specularColor.z;
    d.hasReflective = m.hasReflective;
    d.hasRefractive = m.hasRefractive;
    d.ior = m.indexOfRefraction;
    d.emittance = m.emittance;
    d.invIor = 1.0f / d.ior;
    const float q = (1.0f - d.ior) / (1.0f + d.ior);
    d.r0 = q * q;
    d.invSpecExp1 = m.specularExponent > 0.0f ? 1.0f / (m.specularExponent + 1.0f) : 0.0f;
}

// Pixel rectangle from which camera rays can reach a primitive: project the 8 corners of its object-space unit cube
// (which contains the unit-diameter sphere as well; `box`: a mesh's object-space bounds instead) in double precision.  A camera ray is
//     eye + lambda * (view - right * pixLenX * (px - W/2) - up * pixLenY * (py - H/2)),   px in [x, x+1], py in [y, y+1],
// so a world point Q lies on the ray through continuous pixel (px, py) iff  Q - eye = M * (lambda, lambda sx, lambda sy)
// with M = [view | -pixLenX right | -pixLenY up].  The convex hull of the projected corners contains the projection of
// the primitive; its bounding rectangle is widened by 2 pixels.  Any corner not strictly in front of the eye, or a
// singular M, disables the culling for this primitive (whole frame).
// `hull` (optional): the eight projected corners (continuous pixel coordinates) when the rectangle is a real one, else empty
// What the rectangle must contain is not the primitive but every pixel whose camera ray the REFERENCE's test can report as a hit,
// and that test works in fp32 in object space: seen from R object units away (R large for a small, a distant or a flat
// primitive -- the inverse transform magnifies the eye's coordinates by 1 / scale), the object-space origin carries an absolute error
// ~eps R, the normalised object-space direction ~eps (row sums of the inverse transform x the transform's largest singular value), and the sphere's
// radicand (ro . rd)^2 - (ro . ro - 0.25) ~eps R^2.  A ray that misses the exact primitive by less than that can come back as a hit
// (the device sweep found them at once: a 100 : 1 ellipsoid seen from 20 000 object units through a 1.5-degree lens "hit" from
// pixels 60 columns off its projection).  So the box whose corners are projected is the object-space box INFLATED by those errors, with
// factors on first-order bounds (eps = 2^-24; k = 8 for a cube, 128 for a sphere or a mesh's box):
//     A_i  = sum_j |inv_ij| |eye_j| + |inv_i3|        magnitude of the sums behind ro_i          (error of ro_i   <= 3 eps A_i)
//     B_i  = sum_j |inv_ij|                           ... behind (inverseTransform d)_i, |d| <= 1 (error          <= 3 eps B_i)
//     R    = |A| + 1                                  object-space distance over which a direction error acts
//     D_i  = k eps A_i + R (k eps B_i smax + k eps)    displacement of the computed line along axis i (smax >= the transform's largest
//                                                     singular value: |inverseTransform d| >= |d| / smax)
//     cube / mesh box: half extent + 2 D_i (+ 2e-5 R for a mesh: the relative slack of its slab comparisons), all x (1 + 1e-5)
//     sphere:          the cube of half extent  sqrt(1/4 + 512 eps R^2) + 2 |D|  on every axis
// THE MARGIN, stated like certainMiss's (what is bounded, by which factor, what the sweep saw): the bound is on the distance, in object
// space, by which the EXACT half-line of a camera ray may miss the primitive while the reference's fp32 test still reports a hit.
// pt_test_camera_cull_margin measures it per hit -- the exact half-line in double precision against the primitive grown by a
// fraction s of the inflation -- over the 10 500 (camera, primitive set) pairs of the soundness sweep
// (tests/test_gpu_camera_cull.py::test_inflation_margin_of_the_culling_tables, per primitive type).  Round 3's factors (8 eps, 32 eps R^2:
// "safety factors 2 - 3") turned out to leave the worst SPHERE hit of those cases at s ~ 0.85 of the inflation -- a margin of 1.2 x where
// every other shortcut has 40 - 500 x (0.445 over the first 3000 cases; 0.212 over all of them with the terms x 4, measured on the way).
// Round 4 multiplies the sphere's error terms by SIXTEEN: worst observed fraction 0.105 = a margin of 9.5 x in distance (the case is a
// sphere seen from ~10^4 object units, where the inflation is the radicand's term sqrt(512 eps) R: in that term's factor the margin is
// the square, ~90 x).  CUBES keep round 3's factors: of ~10^9 cube hits in the sweep 18 needed any inflation at all, the worst 0.003 of
// it -- a margin of 300 x -- and the x 16 terms, tried first for every type, made Cornell's thin walls (inverse scale 100 on one axis)
// 0.33 units thick in the tables, ten pixels per side: 7 % of the headline throughput for nothing (profiles/exp_r4l.sh).
// For Cornell's walls that is a fraction of a pixel at 1280 x 720; for the ellipsoid above a hundred pixels; when the inflated box
// reaches the eye, a corner is no longer in front of it and the primitive is not culled at all.
void inflated_object_box(const PtGeom &g, const float *eye, const float *box, double lo[3], double hi[3]) {
    const double eps = 5.9604644775390625e-08;                // 2^-24
    double A[3], B[3], smax2 = 0;
    for (int i = 0; i < 3; ++i) {
        A[i] = std::fabs((double)g.inverseTransform[12 + i]);
        B[i] = 0;
        for (int j = 0; j < 3; ++j) {
            const double m = std::fabs((double)g.inverseTransform[j * 4 + i]);
            A[i] += m * std::fabs((double)eye[j]);
            B[i] += m;
            smax2 += (double)g.transform[j * 4 + i] * (double)g.transform[j * 4 + i];       // Frobenius norm >= largest singular value
        }
    }
    const double smax = std::sqrt(smax2);
    const double R = std::sqrt(A[0] * A[0] + A[1] * A[1] + A[2] * A[2]) + 1.0;
    // (the factor on the first-order terms: 8 for a cube -- measured margin 300 x, below --, 128 for a sphere and for a mesh's box)
    const double kf = (g.type == PT_CUBE && !box) ? 8.0 : 128.0;
    double D[3], Dn = 0;
    for (int i = 0; i < 3; ++i) {
        D[i] = kf * eps * A[i] + R * (kf * eps * B[i] * smax + kf * eps);
        Dn += D[i] * D[i];
    }
    Dn = std::sqrt(Dn);
    for (int i = 0; i < 3; ++i) {
        double l = box ? box[i] : -0.5, h = box ? box[3 + i] : 0.5;
        if (g.type == PT_SPHERE) {
            const double r = std::sqrt(0.25 + 512 * eps * R * R) + 2 * Dn;
            l = -r; h = r;
        } else {
            const double d = 2 * D[i] + (box ? 2e-5 * R : 0.0);
            l -= d; h += d;
        }
        const double c = 0.5 * (l + h), e = 0.5 * (h - l) * (1 + 1e-5);
        lo[i] = c - e;
        hi[i] = c + e;
    }
}

void project_geom(const PtGeom &g, const KParams &k, int rect[4], const float *box = nullptr, std::vector<std::pair<double, double>> *hull = nullptr) {
    if (hull) hull->clear();
    std::vector<std::pair<double, double>> pts;
    rect[0] = rect[1] = 0;
    rect[2] = k.W - 1;
    rect[3] = k.H - 1;
    double blo[3], bhi[3];
    inflated_object_box(g, k.pos, box, blo, bhi);
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(blo[a]) || !std::isfinite(bhi[a])) return;
    const double M[3][3] = {{k.view[0], -(double)k.pixLenX * k.right[0], -(double)k.pixLenY * k.up[0]},
                            {k.view[1], -(double)k.pixLenX * k.right[1], -(double)k.pixLenY * k.up[1]},
                            {k.view[2], -(double)k.pixLenX * k.right[2], -(double)k.pixLenY * k.up[2]}};
    const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                       M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
    double scale = 0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) scale = std::max(scale, std::fabs(M[r][c]));
    if (!(std::fabs(det) > 1e-12 * scale * scale * scale) || !std::isfinite(det)) return;
    double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    for (int corner = 0; corner < 8; ++corner) {
        double o[3];
        for (int a = 0; a < 3; ++a) o[a] = ((corner >> a) & 1) ? bhi[a] : blo[a];       // (the inflated unit cube, or a mesh's inflated box)
        double q[3];
        for (int r = 0; r < 3; ++r)
            q[r] = (double)g.transform[0 + r] * o[0] + (double)g.transform[4 + r] * o[1] + (double)g.transform[8 + r] * o[2] +
                   (double)g.transform[12 + r] - (double)k.pos[r];
        // Cramer: (lambda, lambda sx, lambda sy) = M^-1 q
        double c[3];
        for (int col = 0; col < 3; ++col) {
            double A[3][3];
            for (int r = 0; r < 3; ++r)
                for (int cc = 0; cc < 3; ++cc) A[r][cc] = cc == col ? q[r] : M[r][cc];
            c[col] = (A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                      A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0])) / det;
        }
        const double dist = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
        const double vlen = std::sqrt((double)k.view[0] * k.view[0] + (double)k.view[1] * k.view[1] + (double)k.view[2] * k.view[2]);
        if (!(c[0] * vlen > 1e-3 * dist) || !std::isfinite(c[0])) return;     // corner not clearly in front of the eye
        const double px = c[1] / c[0] + k.halfW, py = c[2] / c[0] + k.halfH;
        if (!std::isfinite(px) || !std::isfinite(py)) return;
        xmin = std::min(xmin, px); xmax = std::max(xmax, px);
        ymin = std::min(ymin, py); ymax = std::max(ymax, py);
        pts.emplace_back(px, py);
    }
    if (hull) *hull = pts;
    auto clampi = [](double v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); };
    rect[0] = clampi(std::floor(xmin) - 2, 0, k.W);
    rect[1] = clampi(std::floor(ymin) - 2, 0, k.H);
    rect[2] = clampi(std::ceil(xmax) + 2, -1, k.W - 1);
    rect[3] = clampi(std::ceil(ymax) + 2, -1, k.H - 1);
}

// Pixels of image row y from which camera rays can reach a primitive whose projected corners are `pts`: the projection of
// the primitive lies in the convex hull of the points, a ray of row y passes the image plane at py in [y, y + 1], so the
// candidates are the x-extent of  hull /\ {y - 2 <= py <= y + 3}  widened by 2 pixels (the rectangle's margins, per row).
// The hull's extent inside a horizontal strip is attained at a vertex inside the strip or where an edge -- of the hull, but
// taking every segment between two of the points only adds points of the hull -- crosses one of the strip's two borders.
// false: the strip misses the hull.
bool hull_row_span(const std::vector<std::pair<double, double>> &pts, int y, double &xmin, double &xmax) {
    const double lo = (double)y - 2.0, hi = (double)y + 3.0;
    xmin = INFINITY; xmax = -INFINITY;
    for (size_t i = 0; i < pts.size(); ++i) {
        if (pts[i].second >= lo && pts[i].second <= hi) { xmin = std::min(xmin, pts[i].first); xmax = std::max(xmax, pts[i].first); }
        for (size_t j = i + 1; j < pts.size(); ++j)
            for (double border : {lo, hi}) {
                const double y0 = pts[i].second, y1 = pts[j].second;
                if ((y0 < border) != (y1 < border)) {
                    const double x = pts[i].first + (pts[j].first - pts[i].first) * ((border - y0) / (y1 - y0));
                    xmin = std::min(xmin, x); xmax = std::max(xmax, x);
                }
            }
    }
    return xmin <= xmax;
}

// Screen-space culling of camera rays, everything pt_init derives from the camera and the primitives' transforms:
//   hg[i].rect   pixel rectangle of primitive i (project_geom),
//   sceneRect    their union: camera rays of pixels outside miss everything (whole tiles are skipped there),
//   rowOff/rowIdx per image row y the primitives whose rectangle covers it, each with the pixels of that row inside the convex
//                hull of its projected corners (hull_row_span): entries {primitive, x0 | x1 << 16}, file order; empty when the
//                frame is too large for the tables (the kernels then use the rectangles).
// Soundness: a primitive lies inside its object-space box, the box inside the convex hull of its eight corners, and a camera ray
// of pixel (x, y) passes the image plane at continuous coordinates in [x, x + 1] x [y, y + 1]; every hit of the reference's tests
// (src/intersections.h:47-143) is a geometric hit of the primitive up to their ~1e-6 relative rounding, which the two pixels of
// margin on every side exceed by orders of magnitude at any supported width (2 px of a 32768-px row is still 6e-5 of the
// image plane).  Whatever cannot be bounded -- a corner not clearly in front of the eye, a singular camera basis -- disables
// the culling for that primitive (whole frame).  `boxes[i]`: object-space bounds of a mesh (6 floats), nullptr otherwise.
// `off`: no culling at all (PT_AMD_NO_CAMERA_CULL, tests only: the reference semantics the culled render must reproduce).
struct CameraCull {
    int sceneRect[4];
    std::vector<int> rowOff, rowIdx;
};
void build_camera_cull(const PtGeom *geoms, int ngeoms, const KParams &k, bool off, const std::vector<const float *> &boxes,
                       std::vector<GeomDev> &hg, CameraCull &cc) {
    const int Wd = k.W, H = k.H;
    cc.sceneRect[0] = cc.sceneRect[1] = 0x7fffffff;   // empty union: a scene without primitives is never entered
    cc.sceneRect[2] = cc.sceneRect[3] = -1;
    cc.rowOff.clear();
    cc.rowIdx.clear();
    std::vector<std::vector<std::pair<double, double>>> hulls(ngeoms ? ngeoms : 1);   // projected corners per primitive
    for (int i = 0; i < ngeoms; ++i) {
        project_geom(geoms[i], k, hg[i].rect, boxes[i], &hulls[i]);
        if (off) {        // (thin lens: rays start anywhere on the lens, the pinhole projection bounds nothing)
            hg[i].rect[0] = hg[i].rect[1] = 0;
            hg[i].rect[2] = Wd - 1;
            hg[i].rect[3] = H - 1;
            hulls[i].clear();
        }
        cc.sceneRect[0] = std::min(cc.sceneRect[0], hg[i].rect[0]);
        cc.sceneRect[1] = std::min(cc.sceneRect[1], hg[i].rect[1]);
        cc.sceneRect[2] = std::max(cc.sceneRect[2], hg[i].rect[2]);
        cc.sceneRect[3] = std::max(cc.sceneRect[3], hg[i].rect[3]);
    }
    if (off || !((long long)H * ngeoms < (1ll << 26) && Wd <= 32768)) return;
    cc.rowOff.resize(H + 1);
    for (int y = 0; y < H; ++y) {
        cc.rowOff[y] = (int)(cc.rowIdx.size() / 2);
        for (int i = 0; i < ngeoms; ++i) {
            if (!(y >= hg[i].rect[1] && y <= hg[i].rect[3] && hg[i].rect[0] <= hg[i].rect[2])) continue;
            int x0 = hg[i].rect[0], x1 = hg[i].rect[2];
            if (!hulls[i].empty()) {
                double xmin, xmax;
                if (!hull_row_span(hulls[i], y, xmin, xmax)) continue;
                x0 = std::max(x0, (int)std::max(std::floor(xmin) - 2.0, -1.0e9));
                x1 = std::min(x1, (int)std::min(std::ceil(xmax) + 2.0, 1.0e9));
                if (x0 > x1) continue;
            }
            cc.rowIdx.push_back(i);
            cc.rowIdx.push_back(x0 | (x1 << 16));
        }
    }
    cc.rowOff[H] = (int)(cc.rowIdx.size() / 2);
    if (cc.rowIdx.empty()) { cc.rowIdx.push_back(0); cc.rowIdx.push_back(0); }
}

// Camera rays as a packed work list (k_bounce<true, ...> of pinhole scenes without meshes or many small primitives): the pixels of this
// shard's rows (y % shardCount == shardRank) that at least one row span of build_camera_cull covers, grouped by their SIGNATURE -- the
// primitives whose spans cover the pixel, file order -- and every group padded to whole waves.  A wave then holds pixels of one
// signature: its lanes all test exactly the primitives the row lists would have let each of them test, none of them idle for another
// lane's primitive, and the frame's pixels that no span covers (misses whatever their jitter) take no lane at all.  Which lane takes
// which pixel changes no result: the camera ray's jitter and the scatter are keyed on the pixel, and the iterations are committed in order.
//   pix     per lane: x | y << 16 (image row y), kCamPad for the padding -- groups padded to 64 lanes, the list to whole tiles (kBlock)
//   wave    per wave of 64 lanes: {first, end} of its signature's primitives in sigIdx (padding waves: an empty range)
//   sigIdx  the signatures' primitives, one run per signature
// false (the kernels keep the row-band tiles): no row lists, a row of more than kCamListRowMax spans (the grouping is quadratic in them),
// more than kCamListSigMax signatures, or a list longer than maxLen lanes (the caller passes the row bands' own index space: the list
// never visits more lanes than the tiles it replaces).  Needs W, H <= 32768 (the pixel word), which the row lists already do.
constexpr int kCamListRowMax = 64, kCamListSigMax = 1 << 16;
struct CameraList {
    std::vector<uint32_t> pix;
    std::vector<int> wave, sigIdx;
    std::vector<int> face;                  // per wave: the cube face its pixels are resolved to (CameraResolve), or -1
    int nSig = 0;
    long long listed = 0;                   // pixels in the list
    long long resolved = 0;                 // ... of them in waves with a face
};

// THE FACE CERTIFICATE of a camera pixel.  A pixel whose signature is one cube g still runs the whole box test (ptd::boxIntersectionTest)
// to learn which of six slab quotients is the answer.  For most such pixels -- the inside of a wall of the room -- the answer is the
// same for every jitter: the ray enters g through one face (K, s), K the axis and s = +-1 the side.  camera_face_certificate says so
// on the host, once per pt_init, and k_bounce<true, ...> then evaluates that one quotient alone (ptd::boxFaceHit).
//
// Pixel (x, y) is RESOLVED to (K, s) of cube g when
//   (i)   the cube's data is tame (CubeCert::ok): every entry finite, |o|_1 <= 2^19 for o = the float32 object-space eye the kernel
//         uses (GeomDev::camObj), the singular values of inverseTransform's linear part L inside [2^-30, 2^30] (bounded by
//         |det L| / |L|_F^2 <= smin, smax <= |L|_F), and the world distance from the eye to the face is clear of rounding:
//         smin(transform) (s o_K - 1/2 - 2e-4) >= 1e-4 (1 + |eye|_1 + |translation|_1 + |transform|_F);
//   (ii)  s o_K >= 1/2 + 1e-2 + inset_K: the eye is outside the slab of axis K, on the side of the face, with room to spare;
//   (iii) each of the four corner directions of the pixel's FOOTPRINT [x - 2, x + 3] x [y - 2, y + 3] (continuous pixel coordinates: the
//         pixel square widened by the spans' own 2 px), q = L (view - right pixLenX (cx - W/2) - up pixLenY (cy - H/2)) in float64,
//         moves towards the face, s q_K < 0 and |q_K| >= 1e-3 |q|, and crosses both planes x_K = s/2 -+ rho (s/2 - o_K), rho = 2^-12 --
//         just in front of the face and just behind it -- at points whose other two coordinates j satisfy |p_j| <= 1/2 - inset_j,
//         inset_j = 8 D_j + 1e-4 with D_j the fp32 displacement of the object-space line along axis j (inflated_object_box's term,
//         its factor 8 for a cube included: four times the allowance the culling tables use, plus an absolute inset).
// Why four corners do: q is affine in (cx, cy), so s q_K < 0 at the corners holds on the whole footprint, and the crossing point with a
// plane x_K = c, p = o + (c - o_K) q / q_K, is a central projection of q: it maps the footprint, a convex set on which the denominator
// keeps its sign, onto a convex quadrilateral whose corners are the corners' images.  The two other slabs' deflated cross-section is
// convex as well, so all four corners inside put every ray of the footprint inside, on both planes.
// What follows for every camera ray of the pixel, jitter in [0, 1)^2, as the reference's loop (src/intersections.h:51-77) evaluates it in
// fp32: its direction is the exact one of some point of the pixel square up to ~1e-6 relative -- orders of magnitude inside the 2 px of
// footprint, the spans' argument -- and its object-space line lies within D of the exact one.  Along the ray, parameter t_K of the face
// plane: at (1 - rho) t_K and at (1 + rho) t_K the point is strictly inside the two other slabs by the inset, so those axes' entry
// parameters lie below (1 - rho) t_K and their exit parameters above (1 + rho) t_K -- rho = 2^-12 against the fast path's doubt margin
// 2^-19 and fp32 rounding ~2^-22.  Axis K's own entry is t_K > 0 (ii) and its exit is later still.  So tmin = t_K with the face
// (K, s), tmax > tmin > 0: a hit, from outside, tmin = RN((s/2 - o_K) / qd_K) -- whether boxSlabsFastDecide or boxSlabsExact got there.
// The ranges: the squared length of L d for a unit d lies in [smin^2, smax^2], inside sqrtUnscaled's and the fast path's [2^-80, 2^80),
// its root inside divUnscaled's exhaustively tested [2^-40, 2^40]; |qd_K| >= ~1e-3 and |s/2 - o_K| in [1e-2, 2^19 + 1] are inside the range
// on which divUnscaled equals IEEE division (tests/test_gpu_parity.py).  Hence the one quotient boxFaceHit forms is bit for bit the
// reference's tmin, and P follows from it by the same operations.  The hit's distance |eye - P| is positive by (i): P lies 1e-4 object
// units in front of the face, at least smin(transform) (s o_K - 1/2 - 1e-4) world units from the eye.
// Whatever cannot be bounded -- a non-finite entry, a singular matrix, an eye inside or near a slab -- leaves the pixel unresolved.
// (the numbers the certificate reads are ptk::FaceCube and ptk::FaceBasis, pt_camera_faces.h: one body for the host and k_camera_faces)
struct CubeCert : FaceCube {
    bool ok = false;
};
struct CameraResolve : FaceBasis {
    std::vector<CubeCert> cube;             // per primitive; ok only for a tame cube
    bool off = false;                       // (PT_AMD_NO_CAMERA_RESOLVE: split as usual, every wave -1)
};
void build_camera_resolve(const PtGeom *geoms, int ngeoms, const KParams &k, const std::vector<GeomDev> &hg, CameraResolve &cr) {
    cr.cube.assign((size_t)(ngeoms > 0 ? ngeoms : 0), CubeCert());
    for (int a = 0; a < 3; ++a) {
        cr.view[a] = k.view[a];
        cr.rx[a] = (double)k.right[a] * (double)k.pixLenX;
        cr.uy[a] = (double)k.up[a] * (double)k.pixLenY;
    }
    cr.halfW = k.halfW;
    cr.halfH = k.halfH;
    const double eps = 5.9604644775390625e-08;                // 2^-24
    for (int i = 0; i < ngeoms; ++i) {
        const PtGeom &g = geoms[i];
        if (g.type != PT_CUBE || (hg[i].flags & 33) != 1) continue;
        CubeCert c;
        bool fin = true;
        double A[3], B[3], F2 = 0, T2 = 0, l1o = 0, l1e = 0, l1t = 0;
        for (int r = 0; r < 3; ++r) {
            c.o[r] = hg[i].camObj[r];
            fin = fin && std::isfinite(c.o[r]);
            l1o += std::fabs(c.o[r]);
            l1e += std::fabs((double)k.pos[r]);
            l1t += std::fabs((double)g.transform[12 + r]);
            A[r] = std::fabs((double)g.inverseTransform[12 + r]);
            B[r] = 0;
            for (int j = 0; j < 3; ++j) {
                c.L[r][j] = hg[i].inv[3 * j + r];
                const double m = std::fabs(c.L[r][j]);
                A[r] += m * std::fabs((double)k.pos[j]);
                B[r] += m;
                F2 += m * m;
                T2 += (double)g.transform[j * 4 + r] * (double)g.transform[j * 4 + r];
            }
        }
        auto det3 = [](double m00, double m01, double m02, double m10, double m11, double m12, double m20, double m21, double m22) {
            return m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) + m02 * (m10 * m21 - m11 * m20);
        };
        const double detL = det3(c.L[0][0], c.L[0][1], c.L[0][2], c.L[1][0], c.L[1][1], c.L[1][2], c.L[2][0], c.L[2][1], c.L[2][2]);
        const double detT = det3(g.transform[0], g.transform[4], g.transform[8], g.transform[1], g.transform[5], g.transform[9],
                                 g.transform[2], g.transform[6], g.transform[10]);
        if (!fin || !std::isfinite(F2) || !std::isfinite(T2) || !std::isfinite(detL) || !std::isfinite(detT) || !(F2 > 0) || !(T2 > 0)) continue;
        const double sminL = std::fabs(detL) / F2, smaxL = std::sqrt(F2), sminT = std::fabs(detT) / T2;
        if (!(sminL >= 0x1p-30) || !(smaxL <= 0x1p+30) || !(l1o <= 0x1p+19) || !(sminT > 0)) continue;
        const double R = std::sqrt(A[0] * A[0] + A[1] * A[1] + A[2] * A[2]) + 1.0, smax = std::sqrt(T2);
        for (int r = 0; r < 3; ++r) {
            const double D = 8.0 * eps * A[r] + R * (8.0 * eps * B[r] * smax + 8.0 * eps);     // (inflated_object_box's D_i, a cube's factor)
            c.inset[r] = kFaceInsetD * D + kFaceInsetAbs;
            fin = fin && std::isfinite(c.inset[r]);       // (an inset of half a unit or more resolves nothing on that axis)
        }
        if (!fin) continue;
        // (the eye's clearance from a face's plane in world units, (i): stored as the least object-space clearance that will do)
        const double need = 1e-4 * (1.0 + l1e + l1t + smax) / sminT + 2e-4;
        if (!std::isfinite(need)) continue;
        c.clear = std::max(kFaceClear, need);
        c.ok = true;
        cr.cube[(size_t)i] = c;
    }
}
// the face (2 K + (s > 0)) pixel (x, y) is resolved to on cube g, or -1
int camera_face_certificate(const CameraResolve &cr, int g, int x, int y) {
    if (g < 0 || (size_t)g >= cr.cube.size() || !cr.cube[(size_t)g].ok) return -1;
    return face_certificate(cr.cube[(size_t)g], cr, x, y);
}

// `cr` (optional): a one-cube signature's pixels are split into the groups its faces resolve (camera_face_certificate) and the
// unresolved rest, each padded to whole waves like a signature; CameraList::face names a wave's face.  A split that makes the list
// longer than maxLen is dropped (every wave -1): the list never visits more lanes than the tiles it replaces.
// The list is built in two passes.  (a) camera_list_groups: the spans are grouped into signature groups of pixels.  (b) camera_list_emit:
// given a face per pixel of every one-cube group whose cube is CubeCert::ok (CameraGroups::faces, one entry per pixel; the other groups'
// stay empty), the stable split by face, the padding to whole waves and the emission.  Between the two, build_camera_list evaluates the
// certificates on the host (camera_list_faces_host); the camera move (pt_api.hip) evaluates them on the device (k_camera_faces) -- the same faces.
struct CameraGroups {
    std::vector<std::vector<uint32_t>> groups;        // per signature its pixels, row-major
    std::vector<std::vector<int>> sigs;
    std::vector<std::vector<int>> faces;              // per group: its pixels' faces, or empty (not a certified one-cube group; no `cr`)
    long long listed = 0, len = 0;                    // pixels in the list; its length without a split
};
// the cube of group s where its pixels get certificates, else -1
int camera_group_cube(const CameraGroups &G, size_t s, const CameraResolve &cr) {
    if (G.sigs[s].size() != 1 || (size_t)G.sigs[s][0] >= cr.cube.size() || !cr.cube[(size_t)G.sigs[s][0]].ok) return -1;
    return G.sigs[s][0];
}
bool camera_list_groups(const CameraCull &cc, int W, int H, int shardRank, int shardCount, long long maxLen, CameraGroups &G) {
    G = CameraGroups();
    if (cc.rowOff.empty() || W > 32768 || H > 32768 || shardCount < 1 || shardRank < 0 || shardRank >= shardCount) return false;
    std::map<std::vector<int>, int> ids;
    std::vector<std::vector<uint32_t>> &groups = G.groups;
    std::vector<std::vector<int>> &sigs = G.sigs;
    std::vector<int> cuts, act;
    for (int y = shardRank; y < H; y += shardCount) {
        const int e0 = cc.rowOff[y], e1 = cc.rowOff[y + 1];
        if (e1 - e0 > kCamListRowMax) return false;
        // the row's spans cut it into runs of one signature: between consecutive span ends
        cuts.clear();
        for (int e = e0; e < e1; ++e) {
            const int sp = cc.rowIdx[2 * e + 1], x0 = std::max(sp & 0xffff, 0), x1 = std::min(sp >> 16, W - 1);
            if (x0 <= x1) { cuts.push_back(x0); cuts.push_back(x1 + 1); }
        }
        std::sort(cuts.begin(), cuts.end());
        cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
        for (size_t c = 0; c + 1 < cuts.size(); ++c) {
            const int a = cuts[c], b = cuts[c + 1];
            act.clear();
            for (int e = e0; e < e1; ++e) {
                const int sp = cc.rowIdx[2 * e + 1];
                if ((sp & 0xffff) <= a && (sp >> 16) >= a) act.push_back(cc.rowIdx[2 * e]);
            }
            if (act.empty()) continue;
            auto it = ids.emplace(act, (int)sigs.size());
            if (it.second) {
                if ((int)sigs.size() >= kCamListSigMax) return false;
                sigs.push_back(act);
                groups.emplace_back();
            }
            std::vector<uint32_t> &g = groups[(size_t)it.first->second];
            for (int x = a; x < b; ++x) g.push_back((uint32_t)x | ((uint32_t)y << 16));
            G.listed += b - a;
        }
    }
    long long len = 0;
    for (const auto &g : groups) len += ((long long)g.size() + 63) / 64 * 64;
    G.len = (len + kBlock - 1) / kBlock * kBlock;
    G.faces.assign(groups.size(), std::vector<int>());
    return G.len <= maxLen;
}
// the host's certificates between the passes: per pixel of every certified one-cube group
void camera_list_faces_host(CameraGroups &G, const CameraResolve &cr) {
    for (size_t s = 0; s < G.groups.size(); ++s) {
        const int cube = camera_group_cube(G, s, cr);
        if (cube < 0) continue;
        const std::vector<uint32_t> &g = G.groups[s];
        std::vector<int> &f = G.faces[s];
        f.resize(g.size());
        for (size_t i = 0; i < g.size(); ++i) f[i] = camera_face_certificate(cr, cube, (int)(g[i] & 0xffffu), (int)(g[i] >> 16));
    }
}
void camera_list_emit(CameraGroups &G, long long maxLen, CameraList &cl, const CameraResolve *cr) {
    cl.pix.clear(); cl.wave.clear(); cl.sigIdx.clear(); cl.face.clear();
    cl.nSig = 0; cl.listed = G.listed; cl.resolved = 0;
    std::vector<std::vector<uint32_t>> &groups = G.groups;
    const std::vector<std::vector<int>> &sigs = G.sigs;
    std::vector<std::vector<int>> &faces = G.faces;
    auto padded = [](long long n) { return (n + 63) / 64 * 64; };
    long long len = G.len;
    // the split of the one-cube signatures: per group its pixels' faces, stably sorted -- the unresolved rest (-1) first, then face by face
    if (cr) {
        long long lenSplit = 0;
        for (size_t s = 0; s < groups.size(); ++s) {
            std::vector<uint32_t> &g = groups[s];
            if (camera_group_cube(G, s, *cr) < 0) {
                lenSplit += padded((long long)g.size());
                continue;
            }
            std::vector<int> &f = faces[s];
            long long n[7] = {0, 0, 0, 0, 0, 0, 0};
            for (size_t i = 0; i < g.size(); ++i) ++n[f[i] + 1];
            std::vector<uint32_t> gs(g.size());
            std::vector<int> fs(g.size());
            size_t at[7], o = 0;
            for (int b = 0; b < 7; ++b) { at[b] = o; o += (size_t)n[b]; lenSplit += padded(n[b]); }
            for (size_t i = 0; i < g.size(); ++i) { const size_t d = at[f[i] + 1]++; gs[d] = g[i]; fs[d] = f[i]; }
            g.swap(gs);
            f.swap(fs);
        }
        lenSplit = (lenSplit + kBlock - 1) / kBlock * kBlock;
        if (lenSplit > maxLen) for (auto &f : faces) f.clear();
        else len = lenSplit;
    } else {
        for (auto &f : faces) f.clear();
    }
    cl.pix.reserve((size_t)len);
    cl.wave.reserve((size_t)len / 32);
    cl.face.reserve((size_t)len / 64);
    for (size_t s = 0; s < groups.size(); ++s) {
        const int first = (int)cl.sigIdx.size();
        cl.sigIdx.insert(cl.sigIdx.end(), sigs[s].begin(), sigs[s].end());
        const int end = (int)cl.sigIdx.size();
        const std::vector<uint32_t> &g = groups[s];
        const std::vector<int> &f = faces[s];
        for (size_t i0 = 0; i0 < g.size();) {          // a run of one face (the whole group where it is not split)
            size_t i1 = g.size();
            const int fc = f.empty() ? -1 : f[i0];
            if (!f.empty()) { i1 = i0; while (i1 < g.size() && f[i1] == fc) ++i1; }
            cl.pix.insert(cl.pix.end(), g.begin() + (long)i0, g.begin() + (long)i1);
            cl.pix.resize((cl.pix.size() + 63) / 64 * 64, kCamPad);
            while (cl.wave.size() < cl.pix.size() / 32) { cl.wave.push_back(first); cl.wave.push_back(end); }
            cl.face.resize(cl.pix.size() / 64, (cr && cr->off) ? -1 : fc);
            if (fc >= 0 && !(cr && cr->off)) cl.resolved += (long long)(i1 - i0);
            i0 = i1;
        }
    }
    cl.pix.resize((size_t)len, kCamPad);
    cl.wave.resize((size_t)len / 32, 0);
    cl.face.resize((size_t)len / 64, -1);
    if (cl.sigIdx.empty()) cl.sigIdx.push_back(0);
    cl.nSig = (int)sigs.size();
}
bool build_camera_list(const CameraCull &cc, int W, int H, int shardRank, int shardCount, long long maxLen, CameraList &cl,
                       const CameraResolve *cr = nullptr) {
    cl.pix.clear(); cl.wave.clear(); cl.sigIdx.clear(); cl.face.clear();
    cl.nSig = 0; cl.listed = 0; cl.resolved = 0;
    CameraGroups G;
    const bool fits = camera_list_groups(cc, W, H, shardRank, shardCount, maxLen, G);
    cl.listed = G.listed;       // (as before the split into passes: a refused list still says how many pixels it had gathered)
    if (!fits) return false;
    if (cr) camera_list_faces_host(G, *cr);
    camera_list_emit(G, maxLen, cl, cr);
    return true;
}

// host mirrors of the glm ops used for the camera basis (same op order as ptd::)
struct H3 { float x, y, z; };
H3 hcross(H3 x, H3 y) { return H3{x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y}; }
H3 hnormalize(H3 a) {
    float d = a.x * a.x + a.y * a.y + a.z * a.z;
    float s = 1.0f / std::sqrt(d);
    return H3{a.x * s, a.y * s, a.z * s};
}

// the camera constants of spec S2 (KParams: basis, pixel lengths, frame size), derived once on the host
void camera_params(const PtCamera &cam, KParams &k) {
    const int Wd = cam.resolution[0], H = cam.resolution[1];
    const H3 view{cam.view.x, cam.view.y, cam.view.z}, up{cam.up.x, cam.up.y, cam.up.z};
    const H3 right = hnormalize(hcross(view, up));
    k.view[0] = view.x; k.view[1] = view.y; k.view[2] = view.z;
    k.up[0] = up.x; k.up[1] = up.y; k.up[2] = up.z;
    k.right[0] = right.x; k.right[1] = right.y; k.right[2] = right.z;
    k.pos[0] = cam.position.x; k.pos[1] = cam.position.y; k.pos[2] = cam.position.z;
    const float kPI = 3.1415926535897932384626422832795028841971f;   // src/utilities.h:12
    const float ys = std::tan(cam.fov[1] * (kPI / 180));             // src/scene.cpp:133 convention
    const float xs = (ys * Wd) / H;
    k.pixLenX = (2.0f * xs) / (float)Wd;
    k.pixLenY = (2.0f * ys) / (float)H;
    k.halfW = (float)Wd * 0.5f;
    k.halfH = (float)H * 0.5f;
    k.W = Wd; k.H = H;
    k.shardRank = 0; k.shardCount = 1;
}

