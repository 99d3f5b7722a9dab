"""The index maths of the wavefront queue layer (csrc/rt_wf_queue.h: fdiv / make_fastdiv, seg_pos,
dense_entry, own_pixel, pack_state / unpack_state) and the node-group packing (pack_group /
unpack_group, csrc/rt_device.h), evaluated on the host: tools/wf_queue_check.cpp is compiled with
plain g++ and answers requests; every comparison is of exact integers.  The counter map
(csrc/rt_wf_counters.h) is checked by its static_asserts, which the tool's build compiles."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARDS = 8


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("wf_queue")), "wf_queue_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__",
                    "-I", ROOT, "-I", os.path.join(rocm, "include"), os.path.join(ROOT, "tools", "wf_queue_check.cpp"),
                    "-o", exe], check=True)

    def run(requests):
        """Answer lines (as lists of ints after the tag) for the request lines."""
        r = subprocess.run([exe], input="".join(q + "\n" for q in requests), capture_output=True, text=True,
                           timeout=60, check=True)
        return [[int(v) for v in line.split()[1:]] if line[:1].isalpha() else [int(v) for v in line.split()]
                for line in r.stdout.split("\n")[:-1]]
    return run


def sweep(d):
    n = [0, 1, d - 1, d, d + 1, 2**31 - 1, 2**31, 2**32 - d, 2**32 - 1]
    n += [k * d + o for k in range(1, 65) for o in (-1, 0, 1)]
    return [v for v in n if v < 2**32]


BIG_D = [2**16 - 1, 2**16, 2**16 + 1, 2**31, 2**32 - 1]


def test_fdiv_every_divisor(ask):
    """fdiv(n, make_fastdiv(d)) == n / d over the sweep, d = 1..4096 and the large divisors."""
    ds = list(range(1, 4097)) + BIG_D
    out = ask([f"D {d}" for d in ds])
    assert len(out) == len(ds)
    for d, (d_out, count, bad) in zip(ds, out):
        assert d_out == d and count == len(sweep(d)), (d, count, len(sweep(d)))
        assert bad == 0, f"d = {d}: {bad} of {count} quotients differ from n / d"


def test_fdiv_values(ask):
    """The same quotients one by one, against Python's n // d: the large divisors and a few small ones."""
    cases = [(d, n) for d in BIG_D + [1, 2, 3, 7, 641, 4095, 4096] for n in sweep(d)]
    out = ask([f"Q {d} {n}" for d, n in cases])
    assert [v[0] for v in out] == [n // d for d, n in cases]


def shard_cases():
    """(seg_cap, L, S) with L[k] + S[k] <= seg_cap: the corner cases and 200 seeded random ones."""
    rng = random.Random(20250)
    cases = []
    for cap in (1, 2, 16, 257):
        cases.append((cap, [0] * SHARDS, [0] * SHARDS))                      # all-zero shards
        cases.append((cap, [cap] * SHARDS, [0] * SHARDS))                    # every front part full
        cases.append((cap, [0] * SHARDS, [cap] * SHARDS))                    # S = seg_cap
        cases.append((cap, [cap, 0, 0, cap, 0, 0, 0, cap], [0, cap, 0, 0, 0, 0, cap, 0]))   # full beside empty
        for _ in range(50):
            L = [rng.choice([0, rng.randint(0, cap), cap]) for _ in range(SHARDS)]
            S = [rng.choice([0, rng.randint(0, cap - l), cap - l]) for l in L]
            cases.append((cap, L, S))
    return cases


def test_dense_entry_and_seg_pos(ask):
    cases = shard_cases()
    assert len(cases) >= 200
    out = ask(["E %d %s %s" % (cap, " ".join(map(str, L)), " ".join(map(str, S))) for cap, L, S in cases])
    assert len(out) == len(cases) * (2 + SHARDS)
    for i, (cap, L, S) in enumerate(cases):
        (n,), dense, per_shard = out[10 * i], out[10 * i + 1], out[10 * i + 2:10 * i + 10]
        front = [[k * cap + j for j in range(L[k])] for k in range(SHARDS)]
        back = [[k * cap + cap - 1 - j for j in range(S[k])] for k in range(SHARDS)]
        assert n == sum(L) + sum(S) == len(dense)
        # every entry exactly once; all front parts in shard order before all back parts
        nf = sum(L)
        assert sorted(dense) == sorted(sum(front, []) + sum(back, [])) and len(set(dense)) == n, (cap, L, S)
        assert dense[:nf] == sum(front, []), (cap, L, S)
        assert dense[nf:] == sum(back, []), (cap, L, S)
        # seg_pos: the same set per shard (front ascending, then back descending)
        for k in range(SHARDS):
            assert per_shard[k] == front[k] + back[k], (cap, L, S, k)


def morton_deinterleave(r):
    x = y = 0
    for b in range(16):
        x |= ((r >> (2 * b)) & 1) << b
        y |= ((r >> (2 * b + 1)) & 1) << b
    return x, y


def test_own_pixel(ask):
    own_tiles = 4
    cases = [(t, tx, rank, nr) for t in (16, 24) for tx in (1, 5) for nr in (1, 3) for rank in range(nr)]
    out = ask([f"O {t} {tx} {rank} {nr} {own_tiles * t * t}" for t, tx, rank, nr in cases])
    for (t, tx, rank, nr), flat in zip(cases, out):
        pix = list(zip(flat[0::2], flat[1::2]))
        assert len(pix) == own_tiles * t * t and len(set(pix)) == len(pix), "own_pixel is not injective"
        for i, (px, py) in enumerate(pix):
            k, r = divmod(i, t * t)
            tid = rank + k * nr
            assert (px // t, py // t) == (tid % tx, tid // tx), (t, tx, rank, nr, i)
            if t == 16:   # Morton order inside a power-of-two tile
                assert (px % t, py % t) == morton_deinterleave(r), (t, tx, rank, nr, i)
            else:         # row-major otherwise
                assert (px % t, py % t) == (r % t, r // t), (t, tx, rank, nr, i)


def test_state_and_group_packing(ask):
    rng = random.Random(7)
    states = [(b, t, s) for b in (0, 1, 255) for t in (0, 1, 255) for s in (0, 1, 65535)]
    states += [(rng.randrange(256), rng.randrange(256), rng.randrange(65536)) for _ in range(200)]
    groups = [(b, f, h) for b in (0, 1, 2**23 - 1) for f in (0, 1) for h in (0, 1, 255)]
    groups += [(rng.randrange(2**23), rng.randrange(2), rng.randrange(256)) for _ in range(200)]
    out = ask([f"S {b} {t} {s}" for b, t, s in states] + [f"G {b} {f} {h}" for b, f, h in groups] + ["R"])
    for (b, t, s), got in zip(states, out):
        assert got == [b | t << 8 | s << 16, b, t, s]
    for (b, f, h), got in zip(groups, out[len(states):]):
        assert got == [b << 9 | f << 8 | h, b, f, h]
    # each field over its whole range, the others at 0 and at their maximum
    count, bad = out[-1]
    assert count == 4 * (2 * 256 + 65536 + 2**23 + 256) and bad == 0
