// rt_trav.h — the stepwise traversal of the compressed 8-wide BVH: one query's state in registers
// (Trav) and one iteration of it (trav_step), shared by wf_trace and wf_finish_step
// (rt_wavefront.hip).  trace8 (rt_device.h) is the same traversal as a serial loop (megakernel,
// host tools).  Host and device: tools/root_mask_check.cpp steps it on the host.
#pragma once
#include "rt_device.h"

namespace rt {

// The state of one query in registers: ray setup, closest hit so far (u = bu / bdet, v = bv / bdet:
// the division happens once, when the query ends), the current node group (child base, flip,
// remaining internal hits), the pending triangles of the last node test, and the LDS stack.
struct Trav {
    RaySetup R;
    float best, bu, bv, bdet;
    uint32_t best_id, g_base, g_hits, t_base, t_mask, t_valid;
    bool g_flip, hit_any;
    int sp;
};

__host__ __device__ __forceinline__ void trav_start(Trav& T, f3 o, f3 d, float tmax) {
    T.R = ray_setup(o, d);
    T.best = tmax;
    T.best_id = 0xffffffffu;
    T.bu = T.bv = 0.0f;
    T.bdet = 1.0f;
    T.g_base = 0;
    T.g_hits = 1;   // virtual group holding the root
    T.g_flip = false;
    T.t_mask = 0;
    T.sp = 0;
    T.hit_any = false;
}

// The start from a root word (rt_device.h): the query begins at the root's result, the state the
// root's node step would have left (the groups, triangles and direction that node8_decode makes of
// the producer's mask), so its first iteration is already the root's leaf triangles or first child.
// A mask of 0 leaves nothing to do: the first trav_step returns at once (a miss / unoccluded).
// A word of 0: the virtual root group, as trav_start.  True if the word was consumed: a counting
// caller counts the root as one node visit.
__host__ __device__ __forceinline__ bool trav_start_root(Trav& T, f3 o, f3 d, float tmax, uint32_t word, const RootHead& H) {
    trav_start(T, o, d, tmax);
    if (!(word & kRootValid)) return false;
    node8_decode(word & 0xffu, H.ew, H.h1, T.R.dneg, T.g_hits, T.t_mask, T.t_valid, T.g_base, T.t_base, T.g_flip);
    return true;
}

// The next node's group / stack bookkeeping and index (the step after the triangles of the last
// node test, or a node step without triangles).
__host__ __device__ __forceinline__ uint32_t next_node(Trav& T, int* stack, bool& overflow) {
    if (!T.g_hits) {
        --T.sp;
        const uint32_t ent = (uint32_t)stack[T.sp * kBlock];
        unpack_group(ent, T.g_base, T.g_flip, T.g_hits);
    }
    const int r = T.g_flip ? highest_bit(T.g_hits) : lowest_bit(T.g_hits);
    T.g_hits &= ~(1u << r);
    if (T.g_hits) {
        if (T.sp < kStackSize) {
            stack[T.sp * kBlock] = (int)pack_group(T.g_base, T.g_flip, T.g_hits);
            ++T.sp;
        } else {
            overflow = true;
        }
    }
    return T.g_base + (uint32_t)r;
}

// The node half of a traversal step: the next node of the current group (or the stack), its five
// 16-B words from global memory, the 8-wide test.
template <bool COUNT>
__host__ __device__ __forceinline__ void node_step(const DevScene& S, Trav& T, int* stack, TraceCounters& tc, bool& overflow,
                                                   float cull) {
    const uint32_t ni = next_node(T, stack, overflow);
    if (COUNT) tc.nodes++;
    const NodeWords w = load_node8(S.nodes8, ni);
    test_node8_words(w, T.R, 0.0f, fminf(cull, T.best), T.g_hits, T.t_mask, T.t_valid, T.g_base, T.t_base, T.g_flip);
}

// One iteration of a query: up to two triangles of the last node test (both fetched before either
// is tested: one memory latency; tested in mask order, so closest-hit updates are those of the
// serial loop), then — for a lane whose triangles ran out in this step, and for every lane without
// triangles — one 8-wide node: the next hit child of the current group in slot order (the node's
// children sorted along its longest axis, reversed for rays going the other way), its five 16-B
// words fetched from global memory (an LDS copy of the top levels measured no faster, DESIGN.md
// §3.5).  Returns true once the query is finished (any-hit: an occluder was found).
// `cull`: the distance bound of the box and triangle tests together with T.best (the lower of the
// two); lower than T.best in the finish kernel's team drain (the closest hit any member of the team
// has found), where T.best stays this lane's own hit.
template <bool COUNT>
__host__ __device__ __forceinline__ bool trav_step(const DevScene& S, Trav& T, bool any, int* stack, TraceCounters& tc,
                                                   bool& overflow, float cull) {
    bool tdone = false;
    if (T.t_mask != 0u) {
        const int k0 = lowest_bit(T.t_mask);
        T.t_mask &= T.t_mask - 1u;
        const bool two = T.t_mask != 0u;
        const int k1 = two ? lowest_bit(T.t_mask) : k0;
        if (two) T.t_mask &= T.t_mask - 1u;
        // each vertex as the ray's (kz, kx, ky) window of its record: three 12-B loads and the id
        // per triangle, all in the slot's 64-B line (rt_device.h); both triangles' loads issue
        // before either test
        const uint32_t kz = (uint32_t)T.R.pre.kz;
        const uint32_t f0 = tri_slot(T.t_base, T.t_valid, k0) * (uint32_t)kTriFloats + kz;
        const uint32_t f1 = tri_slot(T.t_base, T.t_valid, k1) * (uint32_t)kTriFloats + kz;
        const f3 a0 = tri_window_at(S.tris, f0), a1 = tri_window_at(S.tris, f0 + 5u), a2 = tri_window_at(S.tris, f0 + 10u);
        const uint32_t ida = tri_id_at(S.tris, f0 - kz);
        const f3 b0 = tri_window_at(S.tris, f1), b1 = tri_window_at(S.tris, f1 + 5u), b2 = tri_window_at(S.tris, f1 + 10u);   // = a for one triangle
        const uint32_t idb = tri_id_at(S.tris, f1 - kz);
        if (COUNT) tc.tris += two ? 2u : 1u;
        // a triangle the ray hits inside the bound: any-hit ends the query, closest-hit keeps it if
        // it is nearer, or as near with the lower id
        auto accept = [&](float t, float u, float v, float dt, uint32_t id) {
            if (any) {
                T.hit_any = true;
                tdone = true;
            } else if (t < T.best || id < T.best_id) {
                T.best = t;
                T.best_id = id;
                T.bu = u;
                T.bdet = dt;
                T.bv = v;
            }
        };
        // the bound is re-read for every test: a triangle must not be accepted beyond a closer hit
        // found earlier in this step (accept assumes t <= T.best)
        float t, u, v, dt;
        if (intersect_rot(T.R.pre, T.R.o, a0, a1, a2, 0.0f, fminf(cull, T.best), &t, &u, &v, &dt)) accept(t, u, v, dt, ida);
        if (two && !tdone && intersect_rot(T.R.pre, T.R.o, b0, b1, b2, 0.0f, fminf(cull, T.best), &t, &u, &v, &dt))
            accept(t, u, v, dt, idb);
    }
    if (!tdone && T.t_mask == 0u && (T.g_hits != 0u || T.sp > 0)) node_step<COUNT>(S, T, stack, tc, overflow, cull);
    return tdone || (T.t_mask == 0u && T.g_hits == 0u && T.sp == 0);
}

}  // namespace rt
