// shadow_skip_check.cpp — the two host-checkable facts the frame kernels' shadow-ray skip rests on
// (csrc/rt_scatter.h: shadow_is_dark, spot_cone), as a stand-alone host program
// (tests/test_shadow_skip.py compiles it with hipcc --offload-host-only: the header is the kernels').
//
//   shadow_skip_check add N SEED
//       For N random a (finite of any magnitude incl. denormals, +0, ±inf, quiet NaN; never -0)
//       and every c in {+0, -0}^3: a + c, by the f3 addition the kernels accumulate with, has the
//       bits of a in every component, and shadow_is_dark(c) holds.  Then shadow_is_dark is false
//       for N random vectors with one NaN, denormal or other non-zero component among zeros.
//   shadow_skip_check spot FILE
//       FILE holds Light records (128 B each).  For each, spot_cone (what load_tabs stages for a
//       spotlight) and QueryDraws::spot (the query policy, on the spot) equal
//       normalize(direction) / cos_pinned(coneAngle) of the record bit for bit.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../metal4-raytracing_amd/csrc/rt_scatter.h"

using namespace rt;

static uint32_t bits(float x) {
    uint32_t u;
    std::memcpy(&u, &x, 4);
    return u;
}
static float from_bits(uint32_t u) {
    float x;
    std::memcpy(&x, &u, 4);
    return x;
}
static uint64_t rng_state;
static uint32_t rnd() {   // splitmix64, upper half
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) >> 32);
}
// an accumulator component: any float but -0 and a signalling NaN (no arithmetic result is one)
static float rnd_accum() {
    switch (rnd() % 8u) {
        case 0: return 0.0f;
        case 1: return from_bits(0x7f800000u | (rnd() & 0x80000000u));                       // ±inf
        case 2: return from_bits(0x7fc00000u | (rnd() & 0x803fffffu));                       // quiet NaN, any payload
        case 3: return from_bits((rnd() & 0x807fffffu) | 1u);                                // denormal, non-zero
        default: {
            uint32_t u = rnd();
            if ((u & 0x7f800000u) == 0x7f800000u) u &= 0xbfffffffu;                          // finite
            if (u == 0x80000000u) u = 0u;                                                    // never -0
            return from_bits(u);
        }
    }
}

static int check_add(long n, uint64_t seed) {
    rng_state = seed;
    const float z[2] = {0.0f, -0.0f};
    long bad = 0;
    for (long i = 0; i < n; ++i) {
        const f3 a = mk3(rnd_accum(), rnd_accum(), rnd_accum());
        for (int k = 0; k < 8; ++k) {
            const f3 c = mk3(z[k & 1], z[(k >> 1) & 1], z[(k >> 2) & 1]);
            const f3 s = a + c;
            if (!shadow_is_dark(c) || bits(s.x) != bits(a.x) || bits(s.y) != bits(a.y) || bits(s.z) != bits(a.z)) {
                if (bad++ < 5)
                    std::printf("add: a = %08x %08x %08x, c case %d -> %08x %08x %08x\n", bits(a.x), bits(a.y), bits(a.z), k,
                                bits(s.x), bits(s.y), bits(s.z));
            }
        }
    }
    for (long i = 0; i < n; ++i) {   // one component that is not a zero
        float v;
        switch (rnd() % 4u) {
            case 0: v = from_bits(0x7f800001u | (rnd() & 0x807fffffu)); break;   // NaN, quiet or signalling
            case 1: v = from_bits((rnd() & 0x807fffffu) | 1u); break;            // denormal
            case 2: v = from_bits(0x00800000u | (rnd() & 0x80000000u)); break;   // smallest normal
            default: {
                uint32_t u = rnd();
                if ((u & 0x7fffffffu) == 0u) u |= 1u;
                v = from_bits(u);
            }
        }
        float c[3] = {z[rnd() & 1u], z[rnd() & 1u], z[rnd() & 1u]};
        c[rnd() % 3u] = v;
        if (shadow_is_dark(mk3(c[0], c[1], c[2]))) {
            if (bad++ < 5) std::printf("dark: %08x %08x %08x\n", bits(c[0]), bits(c[1]), bits(c[2]));
        }
    }
    std::printf("add: %ld accumulators x 8 zero vectors, %ld non-zero vectors, %ld failures\n", n, n, bad);
    return bad ? 1 : 0;
}

static int check_spot(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) {
        std::printf("spot: cannot open %s\n", path);
        return 1;
    }
    std::vector<Light> lights;
    Light l;
    while (std::fread(&l, sizeof l, 1, f) == 1) lights.push_back(l);
    std::fclose(f);
    const QueryDraws<false> draws{nullptr, lights.data(), {}, {}};
    long bad = 0, spots = 0;
    for (size_t k = 0; k < lights.size(); ++k) {
        const Light& L = lights[k];
        spots += L.type == LightTypeSpotlight;
        const f3 axis = normalize(ldf3(L.direction));
        const float c = cos_pinned(L.coneAngle);
        const SpotCone staged = spot_cone(L), query = draws.spot((int)k, draws.light((int)k));
        for (const SpotCone& s : {staged, query})
            if (bits(s.axis.x) != bits(axis.x) || bits(s.axis.y) != bits(axis.y) || bits(s.axis.z) != bits(axis.z) ||
                bits(s.cos_angle) != bits(c)) {
                if (bad++ < 5) std::printf("spot: record %zu differs\n", k);
            }
    }
    std::printf("spot: %zu records, %ld spotlights, %ld failures\n", lights.size(), spots, bad);
    return (bad || lights.empty()) ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "add")) return check_add(std::atol(argv[2]), std::strtoull(argv[3], nullptr, 10));
    if (argc == 3 && !std::strcmp(argv[1], "spot")) return check_spot(argv[2]);
    std::printf("usage: shadow_skip_check add N SEED | spot FILE\n");
    return 2;
}
