#!/usr/bin/env python3
"""How pq_filter4_kernel ends, by hand-out order of its work units: a greedy list-scheduling model on the CPU.

Input: the stderr of a search on a handle created under CUVS_AMD_SCAN_DEBUG=16778240 (1024 + bit 24) - one line
`[pq_units] <rows> <tail pairs>` per list and `[pq_units] unit_rows <n>` - or, without a file, the synthetic index of the issue
(16384 lists, probing queries ~ gamma with mean 78, list lengths ~ normal around 6104 rows).
Units as fill_units_kernel cuts them: per list ceil(pairs / 128) query blocks x ceil(rows / unit_rows) row chunks of equal length.
Cost of a unit: 32-row subtiles x T(groups); T from --t (wave cycles per subtile at 1, 2, 3, 4 query groups, as the counters
report them), default 2 + groups. 1024 workers (one wave per SIMD) take units greedily; printed: makespan / mean load per order.

usage: unit_order_model.py [log] [--t T1,T2,T3,T4] [--workers 1024] [--seed 0]"""
import argparse
import heapq
import random


def units_of(lists, unit_rows, t, group=128):
    out = []
    for rows, pairs in lists:
        if rows == 0 or pairs == 0:
            continue
        n_ch = -(-rows // unit_rows)
        chunk = (-(-rows // n_ch) + 63) // 64 * 64
        for c in range(n_ch):
            r0, r1 = c * chunk, min(rows, (c + 1) * chunk)
            if r0 >= r1:
                continue
            for p in range(0, pairs, group):
                ng = min(4, -(-min(group, pairs - p) // 32))
                out.append(-(-(r1 - r0) // 32) * t[ng - 1])
    return out


def makespan(costs, workers):
    heap = [0.0] * workers
    for c in costs:
        heapq.heapreplace(heap, heap[0] + c)
    return max(heap)


def cheap_tail(costs, share):
    """list order; the cheapest units worth `share` of the total cost move to the end, largest of those first"""
    total, acc, cut = sum(costs), 0.0, 0.0
    srt = sorted(costs)
    i = 0
    while i < len(srt):   # whole groups of equal cost, cheapest first
        j = i
        while j < len(srt) and srt[j] == srt[i]:
            j += 1
        if acc + srt[i] * (j - i) > share * total:
            break
        acc, cut, i = acc + srt[i] * (j - i), srt[i], j
    head = [c for c in costs if c > cut]
    tail = sorted((c for c in costs if c <= cut), reverse=True)   # (stable: equal costs keep list order)
    return head + tail


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log", nargs="?")
    ap.add_argument("--t", default="3,4,5,6")
    ap.add_argument("--workers", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    t = [float(v) for v in args.t.split(",")]
    rng = random.Random(args.seed)
    unit_rows, lists = 8192, []
    if args.log:
        for line in open(args.log, errors="replace"):
            if not line.startswith("[pq_units]"):
                continue
            f = line.split()
            if f[1] == "unit_rows":
                if lists:
                    break   # (the first search of the log)
                unit_rows = int(f[2])
            else:
                lists.append((int(f[1]), int(f[2])))
    else:
        for _ in range(16384):
            lists.append((max(0, int(rng.gauss(6104, 0.25 * 6104))), int(rng.gammavariate(2.2, 78 / 2.2))))
    costs = units_of(lists, unit_rows, t)
    mean = sum(costs) / args.workers
    print(f"lists {len(lists)}, units {len(costs)} ({len(costs) / max(1, len(lists)):.2f} per list), unit_rows {unit_rows}, T {t}")
    print(f"largest unit / mean load of a worker: {max(costs) / mean:.4f}; units per worker {len(costs) / args.workers:.1f}")
    shuffled = costs[:]
    rng.shuffle(shuffled)
    rows = [("list order", costs), ("random order", shuffled), ("largest first", sorted(costs, reverse=True))]
    for share in (0.10, 0.125, 0.15):
        rows.append((f"list order, cheapest {share:.1%} of the cost last, largest of those first", cheap_tail(costs, share)))
    for name, order in rows:
        print(f"{makespan(order, args.workers) / mean:8.4f}  {name}")


if __name__ == "__main__":
    main()
