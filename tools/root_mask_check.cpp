// Checks the root-word start of the stepwise traversal (csrc/rt_trav.h trav_start_root, csrc/rt_device.h
// root_word / node8_hit_slots / node8_decode) on the host.  For seeded rays against small BVHs built
// with build_bvh2 / collapse_bvh8_dp it steps every query three times -- from the virtual root group
// (trav_start), from the producer's word, and from a word of 0 -- and once with the serial loop trace8,
// closest-hit and any-hit, and compares hit records bit for bit, node visits (the root counted), triangle
// tests and the order of the triangle slots tested.
//
//   root_mask_check <kind> <rays>      kind: leaves | mixed | inner   (the shape of the root)
// prints one line
//   <kind> k_int <k> leaf_tris <n> nodes <n> rays <n> root_miss <n> hits <n> occluded <n> saved_steps <n>
//          bad_hit <n> bad_nodes <n> bad_tris <n> bad_order <n> bad_steps <n> bad_zero <n> bad_serial <n>
// and per ray class (inside, outside, axis, miss, shadow_before, shadow_inside, shadow_beyond) a line
//   class <name> rays <n> root_miss <n> found <n>
// tests/test_root_mask.py compiles it with plain g++ (with csrc/rt_bvh.cpp) and checks the answers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "metal4-raytracing_amd/csrc/rt_trav.h"

using namespace rt;

struct Scene {
    std::vector<float> world;   // 9 floats per triangle
    Bvh8Result b8;
    std::vector<float> recs;
    DevScene S{};
    f3 lo, hi;
};

static void add_tri(std::vector<float>& w, f3 c, float size, std::mt19937& rng) {
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    for (int v = 0; v < 3; ++v) {
        w.push_back(c.x + size * U(rng));
        w.push_back(c.y + size * U(rng));
        w.push_back(c.z + size * U(rng));
    }
}

// clusters of `per` small triangles around well separated centres plus `loose` single large triangles
static std::vector<float> make_tris(int clusters, int per, int loose, uint32_t seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    std::vector<float> w;
    for (int c = 0; c < clusters; ++c) {
        const f3 ctr = mk3((c & 1 ? 8.0f : -8.0f) + U(rng), (c & 2 ? 8.0f : -8.0f) + U(rng), (c & 4 ? 8.0f : -8.0f) + U(rng));
        for (int i = 0; i < per; ++i) add_tri(w, mk3(ctr.x + 2.0f * U(rng), ctr.y + 2.0f * U(rng), ctr.z + 2.0f * U(rng)), 0.3f, rng);
    }
    for (int i = 0; i < loose; ++i) add_tri(w, mk3(6.0f * U(rng), 6.0f * U(rng), 6.0f * U(rng)), 1.5f, rng);
    return w;
}

static void finish_scene(Scene& sc) {
    const uint32_t n = (uint32_t)(sc.world.size() / 9);
    const BvhResult b2 = build_bvh2(sc.world.data(), n, 1, 32);
    sc.b8 = collapse_bvh8_dp(b2, 1.0f, 0.5f);
    sc.recs.assign((size_t)kTriFloats * sc.b8.tri_order.size(), 0.0f);
    for (size_t k = 0; k < sc.b8.tri_order.size(); ++k)
        tri_store(&sc.recs[(size_t)kTriFloats * k], &sc.world[9 * (size_t)sc.b8.tri_order[k]], sc.b8.tri_order[k]);
    sc.S.tris = sc.recs.data();
    sc.S.nodes8 = sc.b8.nodes.data();
    sc.S.num_tris = (int)n;
    sc.S.num_nodes8 = (int)sc.b8.nodes.size();
    sc.lo = mk3(INFINITY, INFINITY, INFINITY);
    sc.hi = mk3(-INFINITY, -INFINITY, -INFINITY);
    for (size_t i = 0; i < sc.world.size(); i += 3) {
        sc.lo = mk3(fminf(sc.lo.x, sc.world[i]), fminf(sc.lo.y, sc.world[i + 1]), fminf(sc.lo.z, sc.world[i + 2]));
        sc.hi = mk3(fmaxf(sc.hi.x, sc.world[i]), fmaxf(sc.hi.y, sc.world[i + 1]), fmaxf(sc.hi.z, sc.world[i + 2]));
    }
}

static int root_k(const Scene& sc) { return sc.b8.nodes[0].axis_k >> 4; }
static int root_leaf_tris(const Scene& sc) { return __builtin_popcount(sc.b8.nodes[0].tri_valid); }

// the first seeded scene whose root has the wanted shape
static bool make_scene(const std::string& kind, Scene& sc) {
    for (uint32_t seed = 1; seed <= 64; ++seed) {
        if (kind == "leaves") {   // two triangles: the root is all leaves
            sc.world = make_tris(0, 0, 2, seed);
        } else if (kind == "mixed") {   // internal children and leaf triangles
            sc.world = make_tris(3 + (int)(seed % 3), 40, 1 + (int)(seed % 4), seed);
        } else if (kind == "inner") {   // eight internal children
            sc.world = make_tris(8, 64, 0, seed);
        } else {
            return false;
        }
        finish_scene(sc);
        const int k = root_k(sc), lt = root_leaf_tris(sc);
        if (kind == "leaves" && k == 0 && lt == 2) return true;
        if (kind == "mixed" && k > 0 && k < 8 && lt > 0) return true;
        if (kind == "inner" && k == 8) return true;
    }
    return false;
}

struct Ray {
    f3 o, d;
    float tmax;   // the shadow ray's; the closest-hit query runs to infinity
    int cls;
};
enum { kInside, kOutside, kAxis, kMiss, kShBefore, kShInside, kShBeyond, kClasses };
static const char* kClassName[kClasses] = {"inside", "outside", "axis", "miss", "shadow_before", "shadow_inside", "shadow_beyond"};

static std::vector<Ray> make_rays(const Scene& sc, int n, uint32_t seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f), U01(0.0f, 1.0f);
    const f3 ctr = (sc.lo + sc.hi) * 0.5f, ext = (sc.hi - sc.lo) * 0.5f;
    const float rad = length(ext);
    auto in_box = [&]() { return mk3(ctr.x + ext.x * U(rng), ctr.y + ext.y * U(rng), ctr.z + ext.z * U(rng)); };
    auto dir = [&]() {
        f3 d;
        do d = mk3(U(rng), U(rng), U(rng));
        while (dot(d, d) < 1e-4f || dot(d, d) > 1.0f);
        return normalize(d);
    };
    auto outside = [&]() { return ctr + dir() * (rad * (1.5f + 2.0f * U01(rng))); };
    // a triangle's centroid: rays aimed there find something
    auto target = [&]() {
        const size_t t = (size_t)(U01(rng) * 0.999f * (float)(sc.world.size() / 9));
        const float* p = &sc.world[9 * t];
        return mk3((p[0] + p[3] + p[6]) / 3.0f, (p[1] + p[4] + p[7]) / 3.0f, (p[2] + p[5] + p[8]) / 3.0f);
    };
    std::vector<Ray> rays;
    for (int i = 0; i < n; ++i) {
        Ray r;
        r.cls = i % kClasses;
        r.tmax = 1.0e30f;
        switch (r.cls) {
        case kInside:
            r.o = in_box();
            r.d = (i & 8) ? normalize(target() - r.o) : dir();
            break;
        case kOutside:
            r.o = outside();
            r.d = normalize(((i & 8) ? target() : in_box()) - r.o);
            break;
        case kAxis: {   // one or two zero direction components, from inside and outside
            const int a = (i / 32) % 3;
            f3 d = dir();
            if (a == 0) d.x = 0.0f;
            if (a == 1) d.y = 0.0f;
            if (a == 2) d.z = 0.0f;
            if (i & 64) {   // two zeros
                if (a == 0) d.y = 0.0f;
                if (a == 1) d.z = 0.0f;
                if (a == 2) d.x = 0.0f;
            }
            if (dot(d, d) < 1e-8f) d = mk3(a == 1 ? 1.0f : 0.0f, a == 2 ? 1.0f : 0.0f, a == 0 ? 1.0f : 0.0f);
            if (i & 128) d = mk3(-0.0f - d.x, -0.0f - d.y, -0.0f - d.z);   // negative zeros too
            r.d = normalize(d);
            // through a triangle's centroid from near (inside the box) or far, or from anywhere
            r.o = (i & 16) ? target() - r.d * ((i & 8) ? 0.5f * U01(rng) : rad * (1.5f + U01(rng))) : (i & 8) ? in_box() : outside();
            break;
        }
        case kMiss: {   // away from the box, or past it
            r.o = outside();
            const f3 away = normalize(r.o - ctr);
            r.d = (i & 8) ? away : normalize(cross(away, dir()) + away * 0.05f);
            break;
        }
        default: {   // shadow rays towards a point of the box from outside (or from inside: "before" then ends at once)
            r.o = (i & 8) ? outside() : in_box();
            const f3 p = in_box();
            const float dist = length(p - r.o);
            r.d = (p - r.o) * (1.0f / dist);
            // the distance at which the ray enters the root box (0 from inside)
            float tn = 0.0f;
            const float oo[3] = {r.o.x, r.o.y, r.o.z}, dd[3] = {r.d.x, r.d.y, r.d.z};
            const float lo[3] = {sc.lo.x, sc.lo.y, sc.lo.z}, hi[3] = {sc.hi.x, sc.hi.y, sc.hi.z};
            for (int a = 0; a < 3; ++a)
                if (fabsf(dd[a]) > 1e-6f) tn = fmaxf(tn, fminf((lo[a] - oo[a]) / dd[a], (hi[a] - oo[a]) / dd[a]));
            r.tmax = r.cls == kShBefore ? tn * (0.25f + 0.7f * U01(rng)) : r.cls == kShInside ? dist : 4.0f * rad + dist;
            break;
        }
        }
        rays.push_back(r);
    }
    return rays;
}

struct Run {
    bool found = false, consumed = false;
    Hit hit{};
    uint32_t nodes = 0, tris = 0, steps = 0;
    std::vector<uint32_t> slots;   // the triangle slots fetched for testing, in order
    bool overflow = false;
};

// one query stepped to its end.  start: 0 = trav_start, 1 = the producer's word, 2 = a word of 0
static Run run_steps(const Scene& sc, const Ray& r, bool any, int start, uint32_t word, std::vector<int>& stack) {
    Run out;
    Trav T;
    TraceCounters tc{0, 0, 0};
    const float tmax = any ? r.tmax : INFINITY;
    if (start == 0) {
        trav_start(T, r.o, r.d, tmax);
    } else {
        const Bvh8Node& n0 = sc.b8.nodes[0];
        RootHead H;
        std::memcpy(&H.ew, &n0.e[0], 4);
        H.h1.x = n0.child_base;
        H.h1.y = n0.tri_base;
        H.h1.z = n0.tri_valid;
        out.consumed = trav_start_root(T, r.o, r.d, tmax, start == 1 ? word : 0u, H);
        if (out.consumed) tc.nodes++;   // the root's visit, made by the producer
    }
    bool done = false;
    while (!done) {
        uint32_t m = T.t_mask;
        for (int k = 0; k < 2 && m; ++k) {
            out.slots.push_back(tri_slot(T.t_base, T.t_valid, lowest_bit(m)));
            m &= m - 1u;
        }
        done = trav_step<true>(sc.S, T, any, stack.data(), tc, out.overflow, T.best);
        ++out.steps;
        if (out.steps > 100000u) break;
    }
    out.found = any ? T.hit_any : T.best_id != 0xffffffffu;
    out.hit.t = T.best;
    out.hit.id = T.best_id;
    out.hit.u = T.bu / T.bdet;
    out.hit.v = T.bv / T.bdet;
    out.nodes = tc.nodes;
    out.tris = tc.tris;
    return out;
}

static bool same_hit(const Run& a, const Run& b, bool any) {
    if (a.found != b.found) return false;
    if (any) return true;
    return std::memcmp(&a.hit, &b.hit, sizeof(Hit)) == 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string kind = argv[1];
    const int nrays = atoi(argv[2]);
    Scene sc;
    if (!make_scene(kind, sc)) {
        fprintf(stderr, "no scene with a root of kind '%s'\n", kind.c_str());
        return 1;
    }
    const NodeWords root = load_node8(sc.S.nodes8, 0u);
    const std::vector<Ray> rays = make_rays(sc, nrays, 20251u);
    std::vector<int> stack((size_t)kStackSize * kBlock), stack8((size_t)kStackSize * kBlock);
    uint64_t root_miss = 0, hits = 0, occluded = 0, saved = 0, queries = 0;
    uint64_t bad_hit = 0, bad_nodes = 0, bad_tris = 0, bad_order = 0, bad_steps = 0, bad_zero = 0, bad_serial = 0;
    uint64_t cls_rays[kClasses] = {}, cls_miss[kClasses] = {}, cls_found[kClasses] = {};
    for (const Ray& r : rays) {
        for (int any = 0; any < 2; ++any) {
            const float tmax = any ? r.tmax : INFINITY;
            const uint32_t word = root_word(root, r.o, r.d, tmax);
            const Run a = run_steps(sc, r, any != 0, 0, 0u, stack);
            const Run b = run_steps(sc, r, any != 0, 1, word, stack);
            const Run z = run_steps(sc, r, any != 0, 2, 0u, stack);
            ++queries;
            const bool miss = (word & 0xffu) == 0u;
            // the shadow query is the one the classes' tmax is about; the closest-hit one for the rest
            if ((r.cls >= kShBefore) == (any != 0)) {
                cls_rays[r.cls]++;
                cls_miss[r.cls] += miss;
                cls_found[r.cls] += a.found;
            }
            root_miss += miss;
            (any ? occluded : hits) += a.found;
            if (!(word & kRootValid) || !b.consumed) ++bad_steps;
            if (!same_hit(a, b, any != 0)) ++bad_hit;
            if (a.nodes != b.nodes) ++bad_nodes;
            if (a.tris != b.tris) ++bad_tris;
            if (a.slots != b.slots) ++bad_order;
            // a root miss: one step that does nothing; else exactly the root's step less
            if (miss ? (b.steps != 1u || b.nodes != 1u || b.tris != 0u || b.found) : (b.steps + 1u != a.steps)) ++bad_steps;
            saved += a.steps - b.steps;
            // a word of 0 is today's start, step for step
            if (z.consumed || !same_hit(a, z, any != 0) || a.nodes != z.nodes || a.tris != z.tris || a.slots != z.slots ||
                a.steps != z.steps)
                ++bad_zero;
            // the serial loop: the same hit and the same counts
            Hit h8{};
            TraceCounters t8{0, 0, 0};
            bool ovf = false;
            const bool f8 = any ? trace8<true, true>(sc.S, r.o, r.d, 0.0f, tmax, h8, stack8.data(), t8, ovf)
                                : trace8<false, true>(sc.S, r.o, r.d, 0.0f, tmax, h8, stack8.data(), t8, ovf);
            bool ok8 = f8 == b.found && t8.nodes == b.nodes;
            if (!any) ok8 = ok8 && std::memcmp(&h8, &b.hit, sizeof(Hit)) == 0 && t8.tris == b.tris;
            if (!ok8) ++bad_serial;
        }
    }
    printf("%s k_int %d leaf_tris %d nodes %zu rays %llu root_miss %llu hits %llu occluded %llu saved_steps %llu "
           "bad_hit %llu bad_nodes %llu bad_tris %llu bad_order %llu bad_steps %llu bad_zero %llu bad_serial %llu\n",
           kind.c_str(), root_k(sc), root_leaf_tris(sc), sc.b8.nodes.size(), (unsigned long long)queries,
           (unsigned long long)root_miss, (unsigned long long)hits, (unsigned long long)occluded, (unsigned long long)saved,
           (unsigned long long)bad_hit, (unsigned long long)bad_nodes, (unsigned long long)bad_tris,
           (unsigned long long)bad_order, (unsigned long long)bad_steps, (unsigned long long)bad_zero,
           (unsigned long long)bad_serial);
    for (int c = 0; c < kClasses; ++c)
        printf("class %s rays %llu root_miss %llu found %llu\n", kClassName[c], (unsigned long long)cls_rays[c],
               (unsigned long long)cls_miss[c], (unsigned long long)cls_found[c]);
    return 0;
}
