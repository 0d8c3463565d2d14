#!/usr/bin/env python3
"""Entropy stage time of the section-per-workgroup kernels, one stream of tests/test_ac_walk.py per route: the 200-table
stream on k_entropy_ans, prefix_lz77 on k_entropy_generic, mixed_520 on k_entropy_uni. Run under JXLHIP_ENTROPY=1 (no
frame takes the lane kernel; the route is asserted). Per stream the minimum of --runs runs of the stage, from the HIP
events around it (jxlhip_last_stage_ms(0)), as one JSON line. --lib names another build of libjxl_amd.so to compare with.
usage: JXLHIP_ENTROPY=1 measure_entropy_fallbacks.py [--lib path] [--runs 20]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
STREAMS = {"k_entropy_ans": ("subsampled0_bctx1_clusters", 2), "k_entropy_generic": ("prefix_lz77", 3), "k_entropy_uni": ("mixed_520", 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    import libjxl_amd as J
    if a.lib:
        J.LIB_PATH = os.path.abspath(a.lib)
    import test_ac_walk as C
    out = {}
    for kernel, (name, route) in STREAMS.items():
        f = J.Frame(C.DECODE_CASES[name](J), threads=2)
        c = J.HipContext()
        try:
            c.upload(f)
            assert c.entropy_route() == route, (kernel, c.entropy_route())
            ms = []
            for _ in range(a.runs + 2):
                c.run_entropy()
                c.sync()
                ms.append(c.stage_ms(0))
            r, flags = c.errors()
            assert r == 0 and not any(flags), kernel
            out[kernel] = round(min(ms[2:]), 4)
        finally:
            c.close()
            f.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
