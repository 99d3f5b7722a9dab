"""Device ray queries against the renderer's own primary-ray traversal: one JSON
line for C3g at 1920x1080.

(a) frame: one frame with debugTextureMode = 1 and samplesPerPixel = 4, graphs off, one frame in
    flight, tail_paths = 1, so that only primary rays are traced, all of them by the extend launch:
    rate = trace_closest_rays / kernel_ms[1].  Reported only if closest_rays == W * H * 4.
(b) query: Renderer.trace on W * H * 4 rays through the pixel centres of camera_default (four per
    pixel; pixels in the frame's order, 64-pixel tiles and Morton order within a tile):
    rate = rays / query_stats().device_ms.

Each is the median of five runs after two warm-up runs, in a child process of its own whose
every run has a time limit (the child is killed when a run does not report in time).  After the
timed runs each child does one counting run for the node visits and triangle tests per ray.

--resolve runs one other leg instead and prints its own JSON line:
(c) resolve: Renderer.resolve on the rays and hit records of (b), with and without material
    records, each timed by HIP events around the launch on its stream (median of five after two
    warm-up runs).  Reported as records per second (Ghits/s; the share of records that are hits
    beside it) and as the fraction of the HBM floor: 64 B of ray and hit in, the 64-B tri_nrm line
    and 64 B (112 B with materials) out per record, at 6.3 TB/s.

--shade runs legs (c, with materials) and (d) in one child and prints one JSON line:
(d) shade: Renderer.shade on the rays, surface and material records of (c) with fresh camera
    paths (throughput 1, bounce 0, Halton index = the ray's number mod 2^20; restored from a copy
    before every run, outside the timed span), the Renderer's default uniforms (PBR, 2 bounces),
    timed the same way.  Reported as records per second and as the fraction of the HBM floor:
    16 B of ray direction, 64 B of surface, 48 B of material and 48 B of path in, 48 B of path,
    two 32-B rays and 16 B of contribution out per record (304 B), at 6.3 TB/s.  Then the same
    launch with the caller's numbers (uniform random, 32 B more per record: 336 B) in place of the
    Halton draws, which tells the cost of the Halton digit loops from that of the traffic.

--loop runs leg (e) in one child and prints one JSON line:
(e) loop: the whole frame (frame 0 at --spp samples and --bounces bounces, the bench's 4 and 8)
    four ways on one build, one renderer, one session: Renderer.path_trace (library calls only:
    camera_paths, then trace / resolve / shade / compact / trace_any / connect / retire / compact
    per round, then average); the torch-glue loop of tests/shade_ref.py integrate / render on the
    device (per sample: boolean-index selection of the shadow rays, torch.where for the add, a
    torch sum for the pixel) in its carry form (dead records kept) and in its boolean-index
    compaction form; and Renderer.draw (rt_render_frame) for scale.  Each is timed by the wall
    clock around one frame that ends with a device synchronisation, median of five after two
    warm-up runs; rate = (closest-hit + shadow rays of the frame) / time.  The three query images
    are compared bit for bit.  Beside them the device-count leg: Renderer.path_trace(device_counts=
    True) at look-ahead 0, 1 and 2 (every launch's count read on the device, one event wait per
    round `lookahead` rounds behind the enqueue), timed the same way in the same session, its image
    compared with the loop's bit for bit (loop_device_ms / loop_device_grays per look-ahead,
    loop_device_host_waits).  Then rt_compact_paths alone on round 0's records of path_trace's
    batch, in the loop's two shapes (SHADOW: shadow rays + index; ALIVE: next rays + paths), timed by
    HIP events on a stream of its own (median of five after two), as a share of its HBM floor at
    6.3 TB/s: every line of `paths` read once for the flag words (48 n), the selection words
    written and read (n / 8 each), m x 16 x words read and the same written, 4 m of index.

    python tools/query_bench.py [--resolve | --shade | --loop] [--scene c3g] [--width 1920] [--height 1080] [--run-timeout 60]
"""
import argparse
import importlib
import json
import os
import selectors
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, RUNS = 2, 5


def _rt():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("metal4-raytracing_amd")


def _emit(**kw):
    print(json.dumps(kw), flush=True)


def child_frame(args):
    rt = _rt()
    W, H = args.width, args.height
    R = rt.Renderer(rt.Scene.preset(args.scene), W, H, tail_paths=1, frames_in_flight=1)
    R.set_graphs(False)
    R.debugTextureMode = 1
    R.samplesPerPixel = 4
    _emit(ready=True)
    for k in range(WARMUP + RUNS + 1):
        counting = k == WARMUP + RUNS
        R.set_counting(counting)
        R.draw()
        s = R.stats()
        if s.closest_rays != W * H * 4 or s.trace_closest_rays != W * H * 4 or s.shadow_rays != 0:
            _emit(error=f"the frame traced {s.closest_rays} closest-hit rays ({s.trace_closest_rays} by the extend "
                        f"launch) and {s.shadow_rays} shadow rays, not {W * H * 4} primary rays only")
            return 1
        if counting:
            _emit(counting=True, nodes_per_ray=s.trace_nodes / s.trace_rays, tris_per_ray=s.trace_tris / s.trace_rays)
        elif not s.kernel_ms[1] > 0:
            _emit(error="the frame recorded no extend time (kernel_ms[1])")
            return 1
        else:
            _emit(run=k, rays=int(s.trace_closest_rays), ms=float(s.kernel_ms[1]))
    R.close()
    return 0


def camera_rays(rt, W, H, device):
    """(W * H * 4, 8) rays through the pixel centres of camera_default, as the kernels form them
    (generate_ray, rt_shade.h), four per pixel, pixels in the frame's order."""
    import numpy as np
    import torch
    ys, xs = np.mgrid[0:H, 0:W]
    tile = (ys // 64) * ((W + 63) // 64) + xs // 64
    lx, ly = (xs % 64).astype(np.uint32), (ys % 64).astype(np.uint32)
    morton = np.zeros_like(lx)
    for b in range(6):
        morton |= ((lx >> b) & 1) << (2 * b) | ((ly >> b) & 1) << (2 * b + 1)
    order = np.lexsort((morton.ravel(), tile.ravel()))
    px = torch.from_numpy(xs.ravel()[order].astype(np.float32)).to(device)
    py = torch.from_numpy(ys.ravel()[order].astype(np.float32)).to(device)
    cam = rt.camera_default(W, H)
    v = lambda f: torch.tensor(f.tolist(), dtype=torch.float32, device=device)
    ux = (px + 0.5) / W * 2.0 - 1.0
    uy = (py + 0.5) / H * 2.0 - 1.0
    d = ux[:, None] * v(cam.right) + uy[:, None] * v(cam.up) + v(cam.forward)
    d = d / d.norm(dim=1, keepdim=True)
    o = v(cam.position).expand_as(d)
    rays = rt.Renderer.make_rays(o, d)
    return rays.repeat_interleave(4, dim=0).contiguous()


def child_query(args):
    rt = _rt()
    import torch
    W, H = args.width, args.height
    R = rt.Renderer(rt.Scene.preset(args.scene), 64, 64)
    rays = camera_rays(rt, W, H, torch.device("cuda", 0))
    out = torch.empty((rays.shape[0], 8), dtype=torch.float32, device=rays.device)
    torch.cuda.synchronize()
    _emit(ready=True)
    for k in range(WARMUP + RUNS + 1):
        counting = k == WARMUP + RUNS
        R.set_counting(counting)
        R.trace(rays, out=out)
        q = R.query_stats()
        if counting:
            _emit(counting=True, nodes_per_ray=q.node_visits / q.rays, tris_per_ray=q.tri_tests / q.rays)
        else:
            _emit(run=k, rays=int(q.rays), ms=float(q.device_ms), hits=int(q.hits), grid_blocks=int(q.grid_blocks))
    R.close()
    return 0


HBM_BYTES_PER_S = 6.3e12   # achievable HBM bandwidth the floor of leg (c) is stated against
RESOLVE_BYTES = {"surface": 64 + 64 + 64, "surface_material": 64 + 64 + 112}   # compulsory bytes per record


def child_resolve(args):
    rt = _rt()
    import torch
    W, H = args.width, args.height
    R = rt.Renderer(rt.Scene.preset(args.scene), 64, 64)
    dev = torch.device("cuda", 0)
    rays = camera_rays(rt, W, H, dev)
    n = rays.shape[0]
    hits = R.trace(rays)
    R.wait()
    surf = torch.empty((n, 16), dtype=torch.float32, device=dev)
    mat = torch.empty((n, 12), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    nhit = int((hits.triangle != -1).sum().item())
    _emit(ready=True)
    for kind, material in (("surface", False), ("surface_material", True)):
        for k in range(WARMUP + RUNS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            R.resolve(rays, hits, material=material, out=(surf, mat) if material else surf, stream=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            _emit(run=k, kind=kind, records=n, hits=nhit, ms=float(e0.elapsed_time(e1)))
    R.close()
    return 0


SHADE_BYTES = (16 + 64 + 48 + 48) + (48 + 32 + 32 + 16)   # compulsory bytes per record of leg (d)


def child_shade(args):
    rt = _rt()
    import torch
    W, H = args.width, args.height
    R = rt.Renderer(rt.Scene.preset(args.scene), 64, 64)
    dev = torch.device("cuda", 0)
    rays = camera_rays(rt, W, H, dev)
    n = rays.shape[0]
    hits = R.trace(rays)
    R.wait()
    surf = torch.empty((n, 16), dtype=torch.float32, device=dev)
    mat = torch.empty((n, 12), dtype=torch.float32, device=dev)
    fresh = rt.Renderer.make_paths(torch.arange(n, device=dev) % (1 << 20)).buffer
    paths = fresh.clone()
    out = (torch.empty((n, 8), dtype=torch.float32, device=dev), torch.empty((n, 8), dtype=torch.float32, device=dev),
           torch.empty((n, 4), dtype=torch.float32, device=dev))
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    nhit = int((hits.triangle != -1).sum().item())
    _emit(ready=True)
    S = None
    rnd = torch.rand((n, 8), generator=torch.Generator(device=dev).manual_seed(1), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    for kind in ("surface_material", "shade", "shade_randoms"):
        for k in range(WARMUP + RUNS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                paths.copy_(fresh)
            e0.record(stream)
            if kind != "surface_material":
                R.shade(rays, S, paths, randoms=rnd if kind == "shade_randoms" else None, out=out, stream=stream.cuda_stream)
            else:
                S = R.resolve(rays, hits, out=(surf, mat), stream=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            _emit(run=k, kind=kind, records=n, hits=nhit, ms=float(e0.elapsed_time(e1)))
    P = rt.Paths(paths, paths.view(torch.int32))
    _emit(shaded=True, alive=int(P.alive.sum().item()), shadow=int(P.shadow.sum().item()))
    R.close()
    return 0


def glue_integrate(rt, R, rays, paths, max_bounces, compact, stream=0):
    """tests/shade_ref.py integrate with its DeviceBackend: the bounce loop over one sample's paths
    with torch between the queries.  Returns (radiance (n, 3), closest rays, shadow rays)."""
    import numpy as np
    import torch
    n, dev = len(paths), rays.device
    index = torch.arange(n, device=dev)
    radiance = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    miss = torch.from_numpy(np.array([0x7F800000, 0, 0] + [0xFFFFFFFF] * 4 + [0], np.uint32).view(np.float32)).to(dev)
    closest = shadow = 0
    guard = max_bounces * (max_bounces + 1) + 1
    for it in range(guard + 1):
        alive = paths.alive
        na = int(alive.sum().item())
        if na == 0:
            break
        if it >= guard:
            raise RuntimeError("a path outlived the renderer's longest")
        if compact:
            radiance[index[~alive]] = paths.radiance[~alive]
            pb = paths.buffer[alive]
            rays, index, paths = rays[alive], index[alive], rt.Paths(pb, pb.view(torch.int32))
            hits = R.trace(rays, stream=stream).buffer
        else:
            hits = miss.expand(n, 8).contiguous()
            hits[alive] = R.trace(rays[alive], stream=stream).buffer
        closest += na
        S = R.resolve(rays, hits, stream=stream)
        out = R.shade(rays, S, paths, stream=stream)
        sh = paths.shadow
        ns = int(sh.sum().item())
        if ns:
            occluded = R.trace(out.shadow_rays[sh], any_hit=True, stream=stream)
            lit = sh.clone()
            lit[sh] = occluded == 0
            paths.radiance[:] = torch.where(lit[:, None], paths.radiance + out.contrib[:, 0:3], paths.radiance)
        shadow += ns
        rays = out.next_rays
    radiance[index] = paths.radiance
    return radiance, closest, shadow


def glue_render(rt, R, spp, max_bounces, compact):
    """tests/shade_ref.py render on the device: per sample the camera records and glue_integrate,
    then pixel = (sum in sample order) / spp.  Returns ((H * W, 3) image, closest, shadow)."""
    total, closest, shadow = None, 0, 0
    u = R.uniforms()
    u.frameIndex = 0
    for s in range(spp):
        rays, paths = R.camera_paths(s, uniforms=u, stream=0)
        rad, nc, ns = glue_integrate(rt, R, rays, paths, max_bounces, compact)
        total = rad if total is None else total + rad
        closest, shadow = closest + nc, shadow + ns
    return total / float(spp), closest, shadow


LOOKAHEADS = (0, 1, 2)   # the device-count leg of --loop
COMPACT_SHAPES = {"shadow": (2, (2,), True), "alive": (1, (2, 3), False)}   # mask, stream words, index


def child_loop(args):
    rt = _rt()
    import torch
    W, H, spp, mb = args.width, args.height, args.spp, args.bounces
    R = rt.Renderer(rt.Scene.preset(args.scene), W, H, frames_in_flight=1)
    R.samplesPerPixel, R.maxBounces = spp, mb
    dev = torch.device("cuda", 0)
    _emit(ready=True)
    images = {}

    def frame():
        R.samplesPerPixel = spp   # resets frameIndex: every run is frame 0
        R.draw()
        R.wait()
        st = R.stats()
        return int(st.closest_rays + st.shadow_rays)

    def loop():
        images["loop"] = R.path_trace()
        t = R.last_path_trace
        return t["closest_rays"] + t["shadow_rays"]

    def glue(compact):
        img, nc, ns = glue_render(rt, R, spp, mb, compact)
        images["glue_compact" if compact else "glue_carry"] = img
        return nc + ns

    waits = {}

    def loop_device(la):
        images[f"loop_device{la}"] = R.path_trace(device_counts=True, lookahead=la)
        t = R.last_path_trace
        waits[la] = t["host_waits"]
        return t["closest_rays"] + t["shadow_rays"]

    legs = [("frame", frame), ("loop", loop), ("glue_carry", lambda: glue(False)), ("glue_compact", lambda: glue(True))]
    legs += [(f"loop_device{la}", lambda la=la: loop_device(la)) for la in LOOKAHEADS]
    for kind, fn in legs:
        for k in range(WARMUP + RUNS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rays = fn()
            torch.cuda.synchronize()
            _emit(run=k, kind=kind, rays=int(rays), ms=(time.perf_counter() - t0) * 1e3)
    rgb = images["loop"].reshape(-1, 4)[:, 0:3].contiguous().view(torch.int32)
    _emit(images=True, equal=bool(torch.equal(rgb, images["glue_carry"].contiguous().view(torch.int32))
                                  and torch.equal(rgb, images["glue_compact"].contiguous().view(torch.int32))),
          device_equal=all(torch.equal(images["loop"].view(torch.int32), images[f"loop_device{la}"].view(torch.int32))
                           for la in LOOKAHEADS),
          rounds=R.last_path_trace["rounds"], host_waits={str(la): waits[la] for la in LOOKAHEADS})
    # round 0 of the batch: every sample's camera paths, traced, resolved and shaded once
    del images
    R._pt_buffers = None
    torch.cuda.empty_cache()
    n = W * H * spp
    rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
    pb = torch.empty((n, 12), dtype=torch.float32, device=dev)
    for s in range(spp):
        R.camera_paths(s, tag_stride=spp, tag_offset=s, out=(rays[s * W * H:(s + 1) * W * H], pb[s * W * H:(s + 1) * W * H]), stream=0)
    out = R.shade(rays, R.resolve(rays, R.trace(rays, stream=0), stream=0), pb, stream=0)
    src = {2: out.shadow_rays, 3: pb}
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    for kind, (mask, words, index) in COMPACT_SHAPES.items():
        streams = [out.next_rays if (w == 2 and kind == "alive") else src[w] for w in words]
        c = R.compact(pb, mask, streams, index=index, stream=stream.cuda_stream)
        m = c.n()
        for k in range(WARMUP + RUNS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            R.compact(pb, mask, streams, index=index, out=c, stream=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            _emit(run=k, kind="compact_" + kind, records=n, selected=m, ms=float(e0.elapsed_time(e1)))
    R.close()
    return 0


def run_child(kind, args):
    """The child's reports; every line has to arrive within its time limit."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--scene", args.scene, "--width", str(args.width),
           "--height", str(args.height), "--spp", str(args.spp), "--bounces", str(args.bounces)]
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE)
    fd = p.stdout.fileno()
    sel = selectors.DefaultSelector()
    sel.register(fd, selectors.EVENT_READ)
    lines, limit = [], args.setup_timeout   # the first report follows the scene load and the BVH build
    buf = b""
    try:
        while True:
            while b"\n" not in buf:
                if not sel.select(timeout=limit):
                    p.kill()
                    return lines, f"{kind}: no report within {limit} s; child killed"
                chunk = os.read(fd, 65536)
                if not chunk:
                    break
                buf += chunk
            if b"\n" not in buf:
                break   # end of the child's output
            line, buf = buf.split(b"\n", 1)
            rec = json.loads(line)
            if "error" in rec:
                return lines, f"{kind}: {rec['error']}"
            lines.append(rec)
            limit = args.run_timeout
    finally:
        sel.close()
        if p.poll() is None:
            try:
                p.wait(timeout=args.run_timeout)
            except subprocess.TimeoutExpired:
                p.kill()
    if p.returncode != 0:
        return lines, f"{kind}: child exited with status {p.returncode}"
    return lines, None


def main_loop(args):
    n = args.width * args.height * args.spp
    res = {"scene": args.scene, "width": args.width, "height": args.height, "spp": args.spp, "bounces": args.bounces, "paths": n,
           "method": f"each leg: {WARMUP} warm-up runs, then the median of {RUNS}; frames by the wall clock around one frame "
                     "ending in a device synchronisation, Grays/s = (closest-hit + shadow rays) / time; compactions by "
                     f"HIP events around the call on its stream, floor at {HBM_BYTES_PER_S / 1e12} TB/s"}
    lines, err = run_child("loop", args)
    legs = (["frame", "loop", "glue_carry", "glue_compact"] + [f"loop_device{la}" for la in LOOKAHEADS]
            + ["compact_" + k for k in COMPACT_SHAPES])
    for kind in legs:
        runs = [r for r in lines if r.get("kind") == kind and r["run"] >= WARMUP]
        if not err and len(runs) != RUNS:
            err = f"loop ({kind}): {len(runs)} timed runs reported, not {RUNS}"
        if err:
            res["error"] = err
            print(json.dumps(res))
            return 1
        res[f"{kind}_ms"] = round(statistics.median(r["ms"] for r in runs), 4)
        res[f"{kind}_runs_ms"] = [round(r["ms"], 4) for r in runs]
        if kind.startswith("compact_"):
            mask, words, index = COMPACT_SHAPES[kind[8:]]
            m = runs[-1]["selected"]
            moved = 16 * sum(words)
            nbytes = 48 * n + 2 * (n // 8) + 2 * m * moved + (4 * m if index else 0)
            res[f"{kind}_selected_share"] = round(m / n, 4)
            res[f"{kind}_floor_bytes"] = nbytes
            res[f"{kind}_floor_ms"] = round(nbytes / HBM_BYTES_PER_S * 1e3, 4)
            res[f"{kind}_floor_fraction"] = round(nbytes / HBM_BYTES_PER_S * 1e3 / res[f"{kind}_ms"], 4)
        else:
            rates = [r["rays"] / r["ms"] * 1e-6 for r in runs]
            res[f"{kind}_rays"] = runs[-1]["rays"]
            res[f"{kind}_grays"] = round(statistics.median(rates), 4)
            res[f"{kind}_runs_grays"] = [round(x, 4) for x in rates]
    for r in lines:
        if r.get("images"):
            res["query_images_bit_equal"] = r["equal"]
            res["loop_rounds"] = r["rounds"]
            res["loop_device_images_bit_equal"] = r["device_equal"]
            res["loop_device_host_waits"] = r["host_waits"]
    # the device-count leg, keyed by look-ahead
    for key in ("ms", "runs_ms", "rays", "grays", "runs_grays"):
        res[f"loop_device_{key}"] = {str(la): res.pop(f"loop_device{la}_{key}") for la in LOOKAHEADS}
    res["loop_device_over_loop"] = {str(la): round(res["loop_device_grays"][str(la)] / res["loop_grays"], 4)
                                    for la in LOOKAHEADS}
    best = max(res["glue_carry_grays"], res["glue_compact_grays"])
    res["loop_over_best_glue"] = round(res["loop_grays"] / best, 4)
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="c3g")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--run-timeout", type=float, default=60.0, help="seconds each run may take")
    ap.add_argument("--setup-timeout", type=float, default=240.0, help="seconds the scene load and BVH build may take")
    ap.add_argument("--resolve", action="store_true", help="leg (c) only: the surface query on leg (b)'s hits")
    ap.add_argument("--shade", action="store_true", help="legs (c, with materials) and (d): the shading query on (c)'s records")
    ap.add_argument("--loop", action="store_true", help="leg (e): the whole frame from queries against the torch-glue loop")
    ap.add_argument("--spp", type=int, default=4, help="--loop: samples per pixel (the bench's 4)")
    ap.add_argument("--bounces", type=int, default=8, help="--loop: bounces (the bench's 8)")
    ap.add_argument("--child", choices=["frame", "query", "resolve", "shade", "loop"])
    args = ap.parse_args()
    if args.child:
        return {"frame": child_frame, "query": child_query, "resolve": child_resolve, "shade": child_shade,
                "loop": child_loop}[args.child](args)
    res = {"scene": args.scene, "width": args.width, "height": args.height, "rays": args.width * args.height * 4}
    if args.loop:
        return main_loop(args)
    if args.resolve or args.shade:
        lines, err = run_child("shade" if args.shade else "resolve", args)
        legs = {"surface_material": RESOLVE_BYTES["surface_material"], "shade": SHADE_BYTES,
                "shade_randoms": SHADE_BYTES + 32} if args.shade else RESOLVE_BYTES
        for kind, nbytes in legs.items():
            runs = [r for r in lines if r.get("kind") == kind and r["run"] >= WARMUP]
            if not err and len(runs) != RUNS:
                err = f"resolve ({kind}): {len(runs)} timed runs reported, not {RUNS}"
            if err:
                res["error"] = err
                print(json.dumps(res))
                return 1
            rates = [r["records"] / r["ms"] * 1e-6 for r in runs]   # records / ms -> Ghits/s
            res[f"{kind}_ghits"] = statistics.median(rates)
            res[f"{kind}_runs_ghits"] = [round(x, 4) for x in rates]
            res[f"{kind}_ms"] = statistics.median(r["ms"] for r in runs)
            res[f"{kind}_floor_ghits"] = round(HBM_BYTES_PER_S / nbytes * 1e-9, 2)
            res[f"{kind}_floor_fraction"] = round(res[f"{kind}_ghits"] * 1e9 * nbytes / HBM_BYTES_PER_S, 4)
            res[f"{kind}_floor_bytes"] = nbytes
            res["hit_share"] = round(runs[-1]["hits"] / runs[-1]["records"], 4)
        for r in lines:
            if r.get("shaded"):
                res["shade_alive_share"] = round(r["alive"] / res["rays"], 4)
                res["shade_shadow_share"] = round(r["shadow"] / res["rays"], 4)
        print(json.dumps(res))
        return 0
    for kind in ("frame", "query"):
        t0 = time.time()
        lines, err = run_child(kind, args)
        if err:
            res["error"] = err
            print(json.dumps(res))
            return 1
        runs = [r for r in lines if "run" in r and r["run"] >= WARMUP]
        if len(runs) != RUNS:
            res["error"] = f"{kind}: {len(runs)} timed runs reported, not {RUNS}"
            print(json.dumps(res))
            return 1
        rates = [r["rays"] / r["ms"] * 1e-6 for r in runs]   # rays / ms -> Grays/s
        res[f"{kind}_grays"] = statistics.median(rates)
        res[f"{kind}_runs_grays"] = [round(x, 4) for x in rates]
        res[f"{kind}_ms"] = statistics.median(r["ms"] for r in runs)
        for r in lines:
            if r.get("counting"):
                res[f"{kind}_nodes_per_ray"] = round(r["nodes_per_ray"], 3)
                res[f"{kind}_tris_per_ray"] = round(r["tris_per_ray"], 3)
        if kind == "query":
            res["query_hits"] = runs[-1]["hits"]
            res["query_grid_blocks"] = runs[-1]["grid_blocks"]
        res[f"{kind}_wall_s"] = round(time.time() - t0, 1)
    res["ratio"] = res["query_grays"] / res["frame_grays"]
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
