// Evaluates the index maths of the wavefront queue layer (csrc/rt_wf_queue.h) and the node-group
// packing (csrc/rt_device.h) on the host, one request per stdin line, one answer line each:
//   Q d n                       -> Q fdiv(n, make_fastdiv(d))
//   D d                         -> D d count bad   fdiv against n / d over the n of the sweep below
//   E cap L0..L7 S0..S7         -> E queue_len, then one line of dense_entry(g) for g < queue_len,
//                                  then one line per shard k of k * cap + seg_pos(g, L[k], cap), g < L[k] + S[k]
//   O tile tiles_x rank nranks n -> O px py px py ...   own_pixel(i) for i < n
//   S bounce tpass step         -> S packed bounce tpass step    (pack_state, unpack_state of it)
//   G base flip hits            -> G packed base flip hits       (pack_group, unpack_group of it)
//   R                           -> R count bad   both round trips over each field's whole range, the others at
//                                  their ends (8 / 8 / 16 bits; 23 / 1 / 8 bits)
// tests/test_wf_queue.py compiles it with plain g++ and checks the answers.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "metal4-raytracing_amd/csrc/rt_device.h"
#include "metal4-raytracing_amd/csrc/rt_wf_queue.h"

// the n of the fdiv sweep for divisor d: 0, 1, d - 1, d, d + 1, every multiple of d within +-1 up to
// 64 d, 2^31 - 1, 2^31, 2^32 - d, 2^32 - 1
static std::vector<uint32_t> sweep(uint32_t d) {
    std::vector<uint32_t> n = {0u, 1u, d - 1u, d, 0x7fffffffu, 0x80000000u, 0u - d, 0xffffffffu};
    if (d != 0xffffffffu) n.push_back(d + 1u);
    for (uint64_t k = 1; k <= 64; ++k)
        for (int o = -1; o <= 1; ++o) {
            const uint64_t v = k * d + o;
            if (v <= 0xffffffffull) n.push_back((uint32_t)v);
        }
    return n;
}

static bool state_ok(int b, int t, int s) {
    const rt::PathState u = rt::unpack_state(rt::pack_state(b, t, s));
    return u.bounce == b && u.tpass == t && u.step == s;
}
static bool group_ok(uint32_t base, bool flip, uint32_t hits) {
    uint32_t b, h;
    bool f;
    rt::unpack_group(rt::pack_group(base, flip, hits), b, f, h);
    return b == base && f == flip && h == hits;
}

int main() {
    char op;
    while (scanf(" %c", &op) == 1) {
        if (op == 'Q') {
            unsigned d, n;
            if (scanf("%u %u", &d, &n) != 2) return 1;
            printf("Q %u\n", rt::fdiv(n, rt::make_fastdiv(d)));
        } else if (op == 'D') {
            unsigned d;
            if (scanf("%u", &d) != 1) return 1;
            const rt::FastDiv f = rt::make_fastdiv(d);
            unsigned bad = 0;
            const std::vector<uint32_t> ns = sweep(d);
            for (uint32_t n : ns) bad += rt::fdiv(n, f) != n / d;
            printf("D %u %zu %u\n", d, ns.size(), bad);
        } else if (op == 'E') {
            unsigned cap;
            rt::QueueShards qs;
            if (scanf("%u", &cap) != 1) return 1;
            for (uint32_t& l : qs.L)
                if (scanf("%u", &l) != 1) return 1;
            for (uint32_t& s : qs.S)
                if (scanf("%u", &s) != 1) return 1;
            const uint32_t n = rt::queue_len(qs);
            printf("E %u\n", n);
            for (uint32_t g = 0; g < n; ++g) printf("%u ", rt::dense_entry(qs, g, cap));
            printf("\n");
            for (int k = 0; k < rt::kShards; ++k) {
                for (uint32_t g = 0; g < qs.L[k] + qs.S[k]; ++g) printf("%u ", k * cap + rt::seg_pos(g, qs.L[k], cap));
                printf("\n");
            }
        } else if (op == 'O') {
            int tile, tiles_x, rank, nranks;
            unsigned n;
            if (scanf("%d %d %d %d %u", &tile, &tiles_x, &rank, &nranks, &n) != 5) return 1;
            rt::PixelMap m;
            m.spp_div = rt::make_fastdiv(1);
            m.tile_px_div = rt::make_fastdiv((uint32_t)tile * (uint32_t)tile);
            m.tiles_x_div = rt::make_fastdiv((uint32_t)tiles_x);
            m.tile = tile;
            m.rank = rank;
            m.nranks = nranks;
            printf("O");
            for (uint32_t i = 0; i < n; ++i) {
                int px, py;
                rt::own_pixel(m, i, px, py);
                printf(" %d %d", px, py);
            }
            printf("\n");
        } else if (op == 'S') {
            int b, t, s;
            if (scanf("%d %d %d", &b, &t, &s) != 3) return 1;
            const uint32_t p = rt::pack_state(b, t, s);
            const rt::PathState u = rt::unpack_state(p);
            printf("S %u %d %d %d\n", p, u.bounce, u.tpass, u.step);
        } else if (op == 'G') {
            unsigned base, flip, hits, b, h;
            bool f;
            if (scanf("%u %u %u", &base, &flip, &hits) != 3) return 1;
            const uint32_t p = rt::pack_group(base, flip != 0, hits);
            rt::unpack_group(p, b, f, h);
            printf("G %u %u %d %u\n", p, b, (int)f, h);
        } else if (op == 'R') {
            unsigned count = 0, bad = 0;
            for (int x = 0; x < 4; ++x) {   // the other two fields at 0 or their maximum
                const bool hi0 = x & 1, hi1 = x & 2;
                for (int v = 0; v < 256; ++v, count += 2) {
                    bad += !state_ok(v, hi0 ? 255 : 0, hi1 ? 65535 : 0);
                    bad += !state_ok(hi0 ? 255 : 0, v, hi1 ? 65535 : 0);
                }
                for (int v = 0; v < 65536; ++v, ++count) bad += !state_ok(hi0 ? 255 : 0, hi1 ? 255 : 0, v);
                for (uint32_t v = 0; v < (1u << 23); ++v, ++count) bad += !group_ok(v, hi0, hi1 ? 255u : 0u);
                for (uint32_t v = 0; v < 256; ++v, ++count) bad += !group_ok(hi0 ? (1u << 23) - 1u : 0u, hi1, v);
            }
            printf("R %u %u\n", count, bad);
        } else {
            return 1;
        }
    }
    return 0;
}
