// Drives the frame ring (csrc/rt_frame_ring.h) from a script on stdin, one operation per line, and
// prints what the ring decides, one line per operation:
//   N                          a new ring (rt_create)                       -> N
//   F nfl wf tile rank nranks  rt_render_frame: plan, begin, commit         -> F slot cross retile_wait ctx_wait flip drain ngens gen motion_prev motion_out
//   U                          a geometry update (begin_update)             -> U seed dst wait_mask   (bit k: slot k)
//   T ctx                      a pack / unpack, on the context's stream (1) or a caller's (0) -> T newest_used
//   C                          other work enqueued on the context's stream  -> C ctx_work
//   R                          rt_resize (after its drain)                  -> R
//   W                          rt_wait: the used slots in harvest order     -> W slot ...
// tests/test_frame_ring.py compiles it with plain g++ and compares against a literal table.
#include <cstdio>

#include "metal4-raytracing_amd/csrc/rt_frame_ring.h"

int main() {
    rt::FrameRing r;
    char op;
    while (scanf(" %c", &op) == 1) {
        if (op == 'N') {
            r = rt::FrameRing();
            printf("N\n");
        } else if (op == 'F') {
            int nfl, wf, tile, rank, nranks;
            if (scanf("%d %d %d %d %d", &nfl, &wf, &tile, &rank, &nranks) != 5) return 1;
            const rt::FramePlan p = r.plan_frame(nfl, wf != 0, tile, rank, nranks);
            r.begin_frame(p);
            r.commit_frame(p);
            printf("F %d %d %d %d %d %d %d %d %d %d\n", p.slot, p.cross, p.retile_wait, p.ctx_wait, p.flip, p.drain,
                   p.ngens, p.gen, p.motion_prev, p.motion_out);
        } else if (op == 'U') {
            const rt::UpdatePlan u = r.plan_update();
            unsigned mask = 0;
            for (int k = 0; k < rt::kMaxSlots; ++k) mask |= (unsigned)u.wait[k] << k;
            if (u.seed) r.commit_update();
            printf("U %d %d %u\n", u.seed, u.dst, mask);
        } else if (op == 'T') {
            int ctx;
            if (scanf("%d", &ctx) != 1) return 1;
            printf("T %d\n", r.newest_used());
            r.tiles_enqueued(ctx != 0);
        } else if (op == 'C') {
            r.ctx_work++;
            printf("C %llu\n", (unsigned long long)r.ctx_work);
        } else if (op == 'R') {
            r.reset_targets();
            printf("R\n");
        } else if (op == 'W') {
            int order[rt::kMaxSlots];
            r.harvest_order(order);
            printf("W");
            for (int k : order)
                if (r.slot[k].used) printf(" %d", k);
            printf("\n");
        } else {
            return 1;
        }
    }
    return 0;
}
