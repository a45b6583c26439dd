#!/usr/bin/env python3
"""The serial chain between consecutive batched voxel updates, from a rocprofv3 kernel-trace rocpd database.
usage: volume_chain.py <db> [frames] [label]
For the last `frames` (default 20) large launches of the batched voxel update - the benchmark's timed window - one table row per frame: the interval from the
end of one update to the start of the next and the time of each volume-chain kernel (garbage collection, list compaction, batch preparation) that ran in it,
then the distribution of the interval and of every chain kernel over the window (markdown, to stdout)."""
import sqlite3
import sys

CHAIN = ["k_gc_identify", "k_gc_delete", "k_gc_finish", "k_compact_count", "k_compact_scatter", "k_list_commit", "k_batch_march", "k_batch_bin", "k_batch_place"]


def short(n):
    return n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0]


def stats(v):
    v = sorted(v)
    if not v:
        return "-"
    m = sum(v) / len(v)
    sd = (sum((x - m) ** 2 for x in v) / len(v)) ** 0.5
    return "n=%d median %.1f mean %.1f sd %.1f min %.1f max %.1f" % (len(v), v[len(v) // 2], m, sd, v[0], v[-1])


def main():
    db = sys.argv[1]
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    label = sys.argv[3] if len(sys.argv) > 3 else db
    c = sqlite3.connect(db)
    rows = [(s, e, short(n)) for s, e, n in c.execute("select start, end, name from kernels order by start")]
    upd = [(s, e) for s, e, n in rows if n.startswith("k_update_batch")]
    if not upd:
        sys.exit("no batched voxel update in the trace")
    big = max(e - s for s, e in upd) * 0.4            # the frame's batch of ~20 operators, not the small batches of the pre-roll's first frames
    upd = [u for u in upd if u[1] - u[0] >= big][-(frames + 1):]
    print("### %s: last %d update-to-update intervals (us)\n" % (label, len(upd) - 1))
    print("| frame | update | interval | " + " | ".join(k[2:] for k in CHAIN) + " | not covered (gaps, hops, waiting) |")
    print("|---|---|---|" + "---|" * (len(CHAIN) + 1))
    per = {k: [] for k in CHAIN}
    gaps, updd = [], []
    for i in range(len(upd) - 1):
        lo, hi = upd[i][1], upd[i + 1][0]
        cell = {}
        for s, e, n in rows:
            if n in per and s < hi and e > lo:
                cell[n] = cell.get(n, 0.0) + (e - s) / 1e3
                per[n].append((e - s) / 1e3)
        g = (hi - lo) / 1e3
        gaps.append(g); updd.append((upd[i][1] - upd[i][0]) / 1e3)
        # what of the interval no chain kernel covers: launch gaps, event hops, waiting for the host (the march may overlap the update: counted where it runs)
        inside = sum(max(0.0, (min(e, hi) - max(s, lo)) / 1e3) for s, e, n in rows if n in per and n != "k_batch_march" and s < hi and e > lo)
        print("| %d | %.0f | %.0f | " % (i, updd[-1], g) + " | ".join("%.0f" % cell[k] if k in cell else "" for k in CHAIN) + " | %.0f |" % (g - inside))
    print("\n- interval: " + stats(gaps))
    print("- update: " + stats(updd))
    for k in CHAIN:
        if per[k]:
            print("- %s: %s" % (k, stats(per[k])))
    span = (upd[-1][1] - upd[0][0]) / 1e6
    print("- window: %.2f ms for %d updates, %.1f us per frame" % (span, len(upd) - 1, span * 1e3 / (len(upd) - 1)))


if __name__ == "__main__":
    main()
