"""CPU count model of the update kernel's per-block LDS table: how many
global upserts (one random key-line probe + one memory-side atomic each) a
launch makes for a given rows-per-block / slots / probes shape.

A block owns `rows_per_block` consecutive rows and inserts their
(key, pane) pairs, in row order, into a table of `slots` entries with
bounded linear probing (`probes` = 1 is the direct-mapped, never-evicting
cache of k_update_batch_n; k_update_tile uses the same hash with more
slots and probes).  A pair that finds no slot sends every one of its rows
to the global table ("LDS-miss rows"); every occupied slot costs one
upsert at the block-end flush.  The in-thread run-collapse, the register
cache and intra-block races are ignored: they mostly catch the hot key.

Plain numpy, no GPU:  python scripts/upsert_model.py [--stream uniform]
The table it prints is the one in profiles/tile_update_note.md."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from arroyo_amd import nexmark  # noqa: E402

NS = 10**9


def hash64(x):
    """splitmix64 finalizer, as hash64() in arroyo_amd.hip (uint64 arrays)."""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9e3779b97f4a7c15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        return x ^ (x >> np.uint64(31))


def lds_home(key, pane, slots):
    """Home slot of (key, pane) in a `slots`-entry LDS table: the hash of
    lds_hot_try / lds_tile_try."""
    with np.errstate(over="ignore"):
        x = key.astype(np.uint64) * np.uint64(2654435761) + \
            pane.astype(np.uint64)
    return (hash64(x) & np.uint64(0xffffffff)).astype(np.int64) & (slots - 1)


def panes_of(ts, slide_ns, ring_panes):
    return (ts.astype(np.uint64) // np.uint64(slide_ns)).astype(np.int64) & \
        (ring_panes - 1)


def simulate(key, pane, rows_per_block, slots, probes):
    """Returns (lds_miss_rows, flush_upserts) over the whole launch."""
    n = len(key)
    home = lds_home(key, pane, slots)
    pair = key.astype(np.int64) * 64 + pane          # panes < 64
    miss = flush = 0
    for lo in range(0, n, rows_per_block):
        hi = min(lo + rows_per_block, n)
        _, first, cnt = np.unique(pair[lo:hi], return_index=True,
                                  return_counts=True)
        used = np.zeros(slots, dtype=bool)
        for i in np.argsort(first):                  # first-occurrence order
            h = int(home[lo + first[i]])
            for p in range(probes):
                s = (h + p) & (slots - 1)
                if not used[s]:
                    used[s] = True
                    flush += 1
                    break
            else:
                miss += int(cnt[i])
    return miss, flush


SHAPES = [  # rows per block, slots, probes
    (2048, 256, 1),
    (2048, 512, 2), (2048, 512, 4),
    (2048, 1024, 2), (2048, 1024, 4),
    (2048, 2048, 2), (2048, 2048, 4),
    (4096, 1024, 4), (4096, 2048, 4),
    (8192, 1024, 4), (8192, 2048, 4),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=54 * 65536,
                    help="rows in the launch (default: one fused bench "
                         "launch, 54 batches of 64K)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--stream", choices=["nexmark", "uniform"],
                    default="nexmark",
                    help="uniform: random keys over 2^20, no time locality")
    ap.add_argument("--slide-s", type=int, default=2)
    ap.add_argument("--ring-panes", type=int, default=16)
    args = ap.parse_args()

    key, ts = nexmark.bids(args.rows, seed=args.seed)
    if args.stream == "uniform":
        rng = np.random.default_rng(args.seed)
        key = rng.integers(0, 1 << 20, size=args.rows).astype(np.int64)
    pane = panes_of(ts, args.slide_s * NS, args.ring_panes)
    n = args.rows
    distinct = len(np.unique(key * 64 + pane))

    print(f"stream={args.stream} rows={n} seed={args.seed}")
    print("| rows per block | LDS slots | probes | LDS-miss rows | "
          "flush upserts | global upserts / row |")
    print("|---|---|---|---|---|---|")
    for rpb, slots, probes in SHAPES:
        miss, flush = simulate(key, pane, rpb, slots, probes)
        print(f"| {rpb} | {slots} | {probes} | {miss:,} | {flush:,} | "
              f"{(miss + flush) / n:.3f} |")
    print(f"| floor: distinct (key, pane) in the launch | | | | "
          f"{distinct:,} | {distinct / n:.3f} |")


if __name__ == "__main__":
    main()
