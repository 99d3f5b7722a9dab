// Checks the exact root boxes (csrc/rt_device.h RootBoxes, root_boxes_fill, root_word_tight) on the host.
// For seeded rays against small BVHs built with build_bvh2 / collapse_bvh8_dp it steps every query twice --
// from the virtual root group (trav_start) and from the tight word (trav_start_root) -- closest-hit and
// any-hit, and compares the hit records bit for bit.  A tight mask of 0 retires the ray in its producer, so
// it must never come with a hit; an empty slot must never get a bit.  Every scene holds a flat quad (a
// floor at y = 0), and the rays around it are the ones the quantised root boxes cannot reject.
//
//   root_tight_check <kind> <rays per class>   kind: leaves | mixed | inner | floor   (the shape of the root)
// prints one line
//   <kind> k_int <k> leaf_tris <n> nodes <n> queries <n> hits <n> occluded <n> retired <n> bad_hit <n> bad_zero <n>
//          bad_empty <n> flat_slot <c or -1> root_extent <y extent> flat_thick <tight y thickness> quant_thick <y>
// and per ray class a line
//   class <name> rays <n> found <n> zero <n> tighter <n> wider <n>
// (rays: queries of the class; zero: tight mask 0; tighter: the tight mask is a strict subset of the quantised
// one; wider: it has a bit the quantised one lacks).  tests/test_root_tight.py compiles it with plain g++
// (with csrc/rt_bvh.cpp) and checks the answers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "metal4-raytracing_amd/csrc/rt_trav.h"

using namespace rt;

constexpr float kFloor = 10.0f;    // the quad: y = 0, x and z in [-kFloor, kFloor]
constexpr float kOffset = 1e-3f;   // a continuation ray's distance from the surface it left

struct Scene {
    std::vector<float> world;   // 9 floats per triangle
    Bvh8Result b8;
    std::vector<float> recs;
    DevScene S{};
    RootBoxes boxes;
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
// the floor as grid x grid cells of two triangles each (1: one quad, a leaf; more: an internal child's worth)
static void add_floor(std::vector<float>& w, int grid) {
    const float s = 2.0f * kFloor / (float)grid;
    for (int i = 0; i < grid; ++i)
        for (int j = 0; j < grid; ++j) {
            const float x0 = -kFloor + s * (float)i, x1 = i + 1 == grid ? kFloor : x0 + s;
            const float z0 = -kFloor + s * (float)j, z1 = j + 1 == grid ? kFloor : z0 + s;
            const float q[18] = {x0, 0, z0, x1, 0, z0, x1, 0, z1, x0, 0, z0, x1, 0, z1, x0, 0, z1};
            w.insert(w.end(), q, q + 18);
        }
}

// the floor, clusters of `per` small triangles around well separated centres above and below it, and `loose`
// single large triangles
static std::vector<float> make_tris(int clusters, int per, int loose, int floor_grid, uint32_t seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    std::vector<float> w;
    add_floor(w, floor_grid);
    for (int c = 0; c < clusters; ++c) {
        const f3 ctr = mk3((c & 1 ? 6.0f : -6.0f) + U(rng), (c & 2 ? 8.0f : -8.0f) + U(rng), (c & 4 ? 6.0f : -6.0f) + U(rng));
        for (int i = 0; i < per; ++i) add_tri(w, mk3(ctr.x + 2.0f * U(rng), ctr.y + 2.0f * U(rng), ctr.z + 2.0f * U(rng)), 0.3f, rng);
    }
    for (int i = 0; i < loose; ++i) add_tri(w, mk3(6.0f * U(rng), 8.0f + 6.0f * U(rng), 6.0f * U(rng)), 1.5f, rng);
    return w;
}

static int root_k(const Scene& sc) { return sc.b8.nodes[0].axis_k >> 4; }
static int root_leaf_tris(const Scene& sc) { return __builtin_popcount(sc.b8.nodes[0].tri_valid); }
static uint32_t root_used(const Scene& sc) {
    uint32_t m = 0;
    for (int c = 0; c < 8; ++c)
        if (!(sc.b8.nodes[0].q[c] == 255 && sc.b8.nodes[0].q[8 + c] == 0)) m |= 1u << c;
    return m;
}
// the root's leaf slot that holds floor triangles only (its box is flat in y before the pad), or -1
static int flat_slot(const Scene& sc) {
    const Bvh8Node& n0 = sc.b8.nodes[0];
    const int k = root_k(sc);
    for (int c = k; c < 8; ++c) {
        if (!((root_used(sc) >> c) & 1u)) continue;
        const uint32_t first = n0.tri_base + bvh8_leaf_first(n0.tri_valid, c - k), n = bvh8_leaf_count(n0.tri_valid, c - k);
        bool flat = n > 0;
        for (uint32_t t = 0; t < n; ++t)
            for (int v = 0; v < 3; ++v) flat = flat && tri_vertex(tri_rec(sc.recs.data(), first + t), v).y == 0.0f;
        if (flat) return c;
    }
    return -1;
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
    root_boxes_fill(sc.boxes, sc.b8.nodes.data(), sc.b8.node_box.data(), sc.recs.data());
    sc.S.root_box = &sc.boxes;
    sc.lo = mk3(INFINITY, INFINITY, INFINITY);
    sc.hi = mk3(-INFINITY, -INFINITY, -INFINITY);
    for (size_t i = 0; i < sc.world.size(); i += 3) {
        sc.lo = mk3(fminf(sc.lo.x, sc.world[i]), fminf(sc.lo.y, sc.world[i + 1]), fminf(sc.lo.z, sc.world[i + 2]));
        sc.hi = mk3(fmaxf(sc.hi.x, sc.world[i]), fmaxf(sc.hi.y, sc.world[i + 1]), fmaxf(sc.hi.z, sc.world[i + 2]));
    }
}

// the first seeded scene whose root has the wanted shape
static bool make_scene(const std::string& kind, Scene& sc) {
    for (uint32_t seed = 1; seed <= 64; ++seed) {
        if (kind == "leaves") {   // the floor and two triangles: the root is all leaves
            sc.world = make_tris(0, 0, 2, 1, seed);
        } else if (kind == "mixed") {   // internal children and leaf triangles
            sc.world = make_tris(3 + (int)(seed % 3), 40, 1 + (int)(seed % 4), 1, seed);
        } else if (kind == "floor") {   // the floor quad as a leaf of a high root
            sc.world = make_tris(2 + (int)(seed % 3), 40, 2, 1, seed + 100u);
        } else if (kind == "inner") {   // eight internal children, the floor (128 triangles) inside them
            sc.world = make_tris(8, 64, 0, 8, seed);
        } else {
            return false;
        }
        finish_scene(sc);
        const int k = root_k(sc), lt = root_leaf_tris(sc);
        if (kind == "leaves" && k == 0 && lt == 4) return true;
        if (kind == "mixed" && k > 0 && k < 8 && lt > 0) return true;
        if (kind == "inner" && k == 8) return true;
        // the floor as a leaf of a root at least 100 times as high as the leaf's box is thick
        if (kind == "floor" && k > 0 && flat_slot(sc) >= 0) return true;
    }
    return false;
}

struct Ray {
    f3 o, d;
    float tmax;   // the any-hit query's; the closest-hit query runs to infinity
};
enum { kAway, kToward, kParallel, kVertex, kEdge, kCorner, kAxis, kShBefore, kShBeyond, kInside, kOutside, kClasses };
static const char* kClassName[kClasses] = {"away", "toward", "parallel", "vertex", "edge", "corner",
                                           "axis", "shadow_before", "shadow_beyond", "inside", "outside"};

static std::vector<Ray> make_rays(const Scene& sc, int cls, int n, uint32_t seed) {
    std::mt19937 rng(seed + 977u * (uint32_t)cls);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f), U01(0.0f, 1.0f);
    const f3 ctr = (sc.lo + sc.hi) * 0.5f, ext = (sc.hi - sc.lo) * 0.5f;
    const float rad = length(ext);
    const size_t ntri = sc.world.size() / 9;
    auto in_box = [&]() { return mk3(ctr.x + ext.x * U(rng), ctr.y + ext.y * U(rng), ctr.z + ext.z * U(rng)); };
    auto dir = [&]() {
        f3 d;
        do d = mk3(U(rng), U(rng), U(rng));
        while (dot(d, d) < 1e-4f || dot(d, d) > 1.0f);
        return normalize(d);
    };
    auto outside = [&]() { return ctr + dir() * (rad * (1.5f + 2.0f * U01(rng))); };
    auto tri = [&]() { return &sc.world[9 * (size_t)(U01(rng) * 0.999f * (float)ntri)]; };
    auto vert = [&](const float* p, int v) { return mk3(p[3 * v], p[3 * v + 1], p[3 * v + 2]); };
    auto on_tri = [&](const float* p) {
        float a = U01(rng), b = U01(rng);
        if (a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }
        return vert(p, 0) * (1.0f - a - b) + vert(p, 1) * a + vert(p, 2) * b;
    };
    auto on_floor = [&]() { return mk3(kFloor * U(rng), 0.0f, kFloor * U(rng)); };
    // outside the scene, anywhere inside it, or kOffset off the floor (side: above / below)
    auto origin = [&](int i, float side) {
        if (i & 8) return outside();
        if (i & 16) return in_box();
        f3 o = on_floor();
        o.y = side * kOffset;
        return o;
    };
    std::vector<Ray> rays;
    for (int i = 0; i < n; ++i) {
        Ray r;
        r.tmax = 1.0e30f;
        const float side = (i & 1) ? 1.0f : -1.0f;   // above / below the floor
        switch (cls) {
        case kAway: case kToward: case kParallel: {   // kOffset off the floor
            r.o = on_floor();
            r.o.y = side * kOffset;
            f3 d = dir();
            d.y = cls == kParallel ? 0.0f : (cls == kAway ? side : -side) * fmaxf(fabsf(d.y), 1e-3f);
            if (dot(d, d) < 1e-8f) d = mk3(1.0f, 0.0f, 0.0f);
            r.d = normalize(d);
            if (cls == kParallel) r.d.y = 0.0f;
            break;
        }
        case kVertex: case kEdge: {   // exactly at a vertex / an edge midpoint
            const float* p = tri();
            const int v = i % 3;
            const f3 target = cls == kVertex ? vert(p, v) : (vert(p, v) + vert(p, (v + 1) % 3)) * 0.5f;
            r.o = origin(i, side);
            r.d = normalize(target - r.o);
            break;
        }
        case kCorner: {   // at a corner of a root child's box
            int c = i % 8;
            while (!((sc.boxes.used >> c) & 1u)) c = (c + 1) % 8;
            const f3 target = mk3(sc.boxes.b[0][(i >> 3) & 1][c], sc.boxes.b[1][(i >> 4) & 1][c], sc.boxes.b[2][(i >> 5) & 1][c]);
            r.o = origin(i >> 3, side);
            r.d = normalize(target - r.o);
            break;
        }
        case kAxis: {   // one or two zero direction components, from near a surface, inside and outside
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
            if (i & 16) r.o = on_tri(tri()) - r.d * ((i & 8) ? 0.5f * U01(rng) : rad * (1.5f + U01(rng)));
            else if (i & 8) r.o = in_box();
            else { r.o = on_floor(); r.o.y = side * kOffset; }
            break;
        }
        case kShBefore: case kShBeyond: {   // shadow rays ending just before / just beyond a triangle
            const f3 p = on_tri(tri());
            r.o = origin(i, side);
            const float dist = length(p - r.o);
            r.d = (p - r.o) * (1.0f / dist);
            r.tmax = dist * (cls == kShBefore ? 1.0f - 1e-4f : 1.0f + 1e-4f);
            break;
        }
        case kInside:
            r.o = (i & 4) ? origin(0, side) : in_box();
            r.d = (i & 8) ? normalize(on_tri(tri()) - r.o) : dir();
            break;
        default:
            r.o = outside();
            r.d = (i & 16) ? dir() : normalize(((i & 8) ? on_tri(tri()) : in_box()) - r.o);
            break;
        }
        rays.push_back(r);
    }
    return rays;
}

struct Run {
    bool found = false;
    Hit hit{};
};

// one query stepped to its end, from the virtual root group (tight = false) or from the tight word
static Run run_steps(const Scene& sc, const Ray& r, bool any, bool tight, uint32_t word, std::vector<int>& stack) {
    Run out;
    Trav T;
    TraceCounters tc{0, 0, 0};
    const float tmax = any ? r.tmax : INFINITY;
    if (!tight) {
        trav_start(T, r.o, r.d, tmax);
    } else {
        const Bvh8Node& n0 = sc.b8.nodes[0];
        RootHead H;
        std::memcpy(&H.ew, &n0.e[0], 4);
        H.h1.x = n0.child_base;
        H.h1.y = n0.tri_base;
        H.h1.z = n0.tri_valid;
        trav_start_root(T, r.o, r.d, tmax, word, H);
    }
    bool overflow = false;
    for (uint32_t steps = 0; steps < 100000u; ++steps)
        if (trav_step<true>(sc.S, T, any, stack.data(), tc, overflow, T.best)) break;
    out.found = any ? T.hit_any : T.best_id != 0xffffffffu;
    out.hit.t = T.best;
    out.hit.id = T.best_id;
    out.hit.u = T.bu / T.bdet;
    out.hit.v = T.bv / T.bdet;
    return out;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string kind = argv[1];
    const int per_class = atoi(argv[2]);
    Scene sc;
    if (!make_scene(kind, sc)) {
        fprintf(stderr, "no scene with a root of kind '%s'\n", kind.c_str());
        return 1;
    }
    const NodeWords root = load_node8(sc.S.nodes8, 0u);
    const uint32_t used = root_used(sc);
    std::vector<int> stack((size_t)kStackSize * kBlock);
    uint64_t queries = 0, hits = 0, occluded = 0, retired = 0, bad_hit = 0, bad_zero = 0, bad_empty = 0;
    uint64_t cls_rays[kClasses] = {}, cls_found[kClasses] = {}, cls_zero[kClasses] = {}, cls_tighter[kClasses] = {},
             cls_wider[kClasses] = {};
    for (int cls = 0; cls < kClasses; ++cls) {
        for (const Ray& r : make_rays(sc, cls, per_class, 20251u)) {
            for (int any = 0; any < 2; ++any) {
                const float tmax = any ? r.tmax : INFINITY;
                const uint32_t quant = root_word(root, r.o, r.d, tmax) & 0xffu;
                const uint32_t word = root_word_tight(sc.boxes, r.o, r.d, tmax);
                const uint32_t mask = word & 0xffu;
                const Run a = run_steps(sc, r, any != 0, false, 0u, stack);
                const Run b = run_steps(sc, r, any != 0, true, word, stack);
                ++queries;
                cls_rays[cls]++;
                cls_found[cls] += a.found;
                cls_zero[cls] += mask == 0u;
                cls_tighter[cls] += (mask & ~quant) == 0u && mask != quant;
                cls_wider[cls] += (mask & ~quant) != 0u;
                (any ? occluded : hits) += a.found;
                if (!any && mask == 0u) ++retired;
                if (!(word & kRootValid) || a.found != b.found || (!any && std::memcmp(&a.hit, &b.hit, sizeof(Hit)) != 0)) ++bad_hit;
                if (mask == 0u && a.found) ++bad_zero;
                if (mask & ~used) ++bad_empty;
            }
        }
    }
    const int fs = flat_slot(sc);
    float flat_thick = 0.0f, quant_thick = 0.0f;
    if (fs >= 0) {
        const Bvh8Node& n0 = sc.b8.nodes[0];
        flat_thick = sc.boxes.b[1][1][fs] - sc.boxes.b[1][0][fs];
        quant_thick = (float)(n0.q[16 + 8 + fs] - n0.q[16 + fs]) * std::ldexp(1.0f, (int)n0.e[1] - 127);
    }
    printf("%s k_int %d leaf_tris %d nodes %zu queries %llu hits %llu occluded %llu retired %llu bad_hit %llu bad_zero %llu "
           "bad_empty %llu flat_slot %d root_extent %g flat_thick %g quant_thick %g\n",
           kind.c_str(), root_k(sc), root_leaf_tris(sc), sc.b8.nodes.size(), (unsigned long long)queries,
           (unsigned long long)hits, (unsigned long long)occluded, (unsigned long long)retired, (unsigned long long)bad_hit,
           (unsigned long long)bad_zero, (unsigned long long)bad_empty, fs, sc.hi.y - sc.lo.y, flat_thick, quant_thick);
    for (int c = 0; c < kClasses; ++c)
        printf("class %s rays %llu found %llu zero %llu tighter %llu wider %llu\n", kClassName[c], (unsigned long long)cls_rays[c],
               (unsigned long long)cls_found[c], (unsigned long long)cls_zero[c], (unsigned long long)cls_tighter[c],
               (unsigned long long)cls_wider[c]);
    return 0;
}
