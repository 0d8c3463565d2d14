"""When do the workgroups of the batched k_entropy_lanes launches start and end?

Runs bench.py's default schedule (two frame sets, three launches per step: filter(A) | entropy(A) | transform(B)) for a few
steps under JXLHIP_LANES_PROF=2: the instrumented form of the kernel stores every wave's first and last instruction on the
clock all XCDs share (100 MHz) and where it ran; the launches are not waited for, so they overlap as they do unprofiled.
For each launch of the timed steps it prints, per XCC and per distinct stream, the first and last start and the first and
last end, in ms from the launch's first start.

usage: entropy_slot_timeline.py [--batch 640] [--size 3840x2160] [--steps 6] [--warmup 2] [--distinct 8]
       (JXLHIP_WG_ORDER=0 / 1 / 2 in the environment selects the order under observation)
"""
import argparse
import os
import sys

os.environ["JXLHIP_LANES_PROF"] = "2"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

TICKS_PER_MS = 1e5


def spans(start, end, t0):
    return "n %4d  start %7.2f .. %7.2f  end %7.2f .. %7.2f" % (len(start), (start.min() - t0) / TICKS_PER_MS, (start.max() - t0) / TICKS_PER_MS,
                                                             (end.min() - t0) / TICKS_PER_MS, (end.max() - t0) / TICKS_PER_MS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=640)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--distinct", type=int, default=8)
    args = ap.parse_args()
    if args.steps > 16:
        raise SystemExit("the library keeps the records of eight launches per frame set: at most 16 steps")
    xsize, ysize = (int(v) for v in args.size.split("x"))
    import libjxl_amd as J
    J.lib()
    datas = [J.encode_rgb8(J.synth_image(xsize, ysize, 177 + i), distance=1.0, strategy_mode=1) for i in range(args.distinct)]
    frames = [J.Frame(d, threads=min(8, os.cpu_count() or 1)) for d in datas]
    sets = [[J.HipContext(0) for _ in range(args.batch)] for _ in range(2)]
    for cs in sets:
        cs[0].set_option("filter_async", 1)
        cs[0].set_option("entropy_gate", 1)
    nth = 0
    for cs in sets:
        for c in cs:
            c.upload(frames[nth % len(frames)])
            nth += 1
    for cs in sets:
        J.run_entropy_batch(cs)
    for cs in sets:
        for c in cs:
            c.sync()
    launches = []  # (step, set) of every entropy launch, in order
    for k in range(args.warmup + args.steps):
        ent, down = sets[k % 2], sets[(k + 1) % 2]
        J.run_filter_color_batch(ent)
        J.run_entropy_batch(ent)
        J.run_transform_batch(down)
        launches.append((k, k % 2))
    for cs in sets:
        for c in cs:
            c.sync()
    print("order JXLHIP_WG_ORDER=%s  batch %d  %dx%d  distinct %d  (ms from each launch's first start; `since` = its first start after the "
          "first start of the launch before it)" % (os.environ.get("JXLHIP_WG_ORDER", "1"), args.batch, xsize, ysize, args.distinct))
    prev_t0 = None
    per_set_seen = [0, 0]
    records = []
    for k, s in reversed(launches):  # back = 0 is a set's last launch
        if k >= args.warmup:
            records.append((k, s, sets[s][0].entropy_timeline(per_set_seen[s])))
        per_set_seen[s] += 1
    for k, s, rec in reversed(records):
        unit, est = sets[s][0].entropy_order()
        assert len(unit) == len(rec)
        one_unit_per_frame = int(unit.max()) + 1 == args.batch
        start, end, xcc = rec[:, 1].astype(np.int64), rec[:, 7].astype(np.int64), (rec[:, 6] >> np.uint64(32)).astype(np.int64) & 15
        t0 = start.min()
        print("step %d set %d: workgroups %d  since %s  all started by %.2f ms  90%% by %.2f ms  last end %.2f ms"
              % (k, s, len(rec), "-" if prev_t0 is None else "%.2f ms" % ((t0 - prev_t0) / TICKS_PER_MS), (start.max() - t0) / TICKS_PER_MS,
                 (np.sort(start)[int(len(start) * 0.9)] - t0) / TICKS_PER_MS, (end.max() - t0) / TICKS_PER_MS))
        prev_t0 = t0
        for x in sorted(set(xcc.tolist())):
            m = xcc == x
            print("  xcc %d     %s" % (x, spans(start[m], end[m], t0)))
        if one_unit_per_frame:
            stream = unit.astype(np.int64) % len(frames)
            # who shares a CU: HW_ID bits 8-15 are the CU, shader array and shader engine inside the XCC
            cu = xcc * 256 + ((rec[:, 6] >> np.uint64(8)).astype(np.int64) & 255)
            length = end - start
            slowest = np.argsort(-np.array([length[stream == d].mean() for d in range(len(frames))]))[:2]
            same = both = 0
            for c in set(cu.tolist()):
                here = stream[cu == c]
                same += len(here) > 1 and len(set(here.tolist())) == 1
                both += int(np.isin(here, slowest).sum() >= 2)
            last = np.argsort(-end)[:16]  # the sixteen workgroups that end last: how many others shared their CUs
            mates = [int((cu == cu[w]).sum()) - 1 for w in last]
            mate_slow = [int(np.isin(stream[(cu == cu[w])], slowest).sum()) - int(stream[w] in slowest) for w in last]
            print("  CUs used %d (with 1 / 2 / 3+ workgroups: %s); CUs whose workgroups are all one stream %d; CUs with two or more of the two "
                  "slowest streams %d; the 16 last to end shared their CU with %.2f others on average, %.2f of them of the two slowest streams"
                  % (len(set(cu.tolist())), " / ".join(str(int((np.bincount(np.unique(cu, return_inverse=True)[1]) == k).sum())) for k in (1, 2))
                     + " / " + str(int((np.bincount(np.unique(cu, return_inverse=True)[1]) >= 3).sum())), same, both, np.mean(mates), np.mean(mate_slow)))
            for d in range(len(frames)):
                m = stream == d
                print("  stream %d  %s  length %6.2f .. %6.2f  xccs %s" % (d, spans(start[m], end[m], t0), (end[m] - start[m]).min() / TICKS_PER_MS,
                                                                        (end[m] - start[m]).max() / TICKS_PER_MS, sorted(set(xcc[m].tolist()))))
    for cs in sets:
        for c in cs:
            c.close()


if __name__ == "__main__":
    main()
