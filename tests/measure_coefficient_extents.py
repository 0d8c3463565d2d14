"""CPU statistics of the benchmark's own streams for the transform kernel's shortcuts: per varblock class
the share of pixels, the mean kend / size per channel, the staging rounds no varblock of a wave reaches and the waves whose
X and B have no AC at all. No GPU: the oracle decodes the streams with dumps, kend comes from its coefficients through the
natural coefficient order (coefficient_extents.py).

    python3 tests/measure_coefficient_extents.py [--size 3840x2160] [--distance 1.0] [--seeds 177,181]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--distance", type=float, default=1.0)
    ap.add_argument("--seeds", default="177,181")
    args = ap.parse_args()
    import libjxl_amd as J
    import jxlo
    import coefficient_extents as E
    J.build()
    jxlo.build()
    xs, ys = (int(v) for v in args.size.split("x"))
    for seed in (int(v) for v in args.seeds.split(",")):
        data = J.encode_rgb8(J.synth_image(xs, ys, seed), distance=args.distance, strategy_mode=1)  # (bench.py's stream)
        o = jxlo.Decoded(data)
        dec = E.wave_decisions(E.oracle_extents(o))
        o.close()
        pixels = sum(d["positions"] for d in dec.values())
        print("seed %d: %d bytes, %d varblocks of the fast transform kernel" % (seed, len(data), sum(d["blocks"] for d in dec.values())))
        print("%-7s %7s  %-20s %9s %9s  %s" % ("class", "pixels", "mean kend/size X Y B", "rounds", "left out", "waves with X / B from the corner alone"))
        tot_rounds = tot_skipped = tot_kend = 0
        for st in sorted(dec, key=lambda s: -dec[s]["positions"]):
            d = dec[st]
            ke = [k / d["positions"] for k in d["kend_sum"]]
            tot_rounds += d["rounds"]
            tot_skipped += d["skipped_rounds"]
            tot_kend += sum(d["kend_sum"])
            print("%-7s %6.1f%%  %.3f %.3f %.3f    %9d %8.1f%%  %5.1f%% / %5.1f%%  (%d waves)" % (
                E.NAMES[st], 100.0 * d["positions"] / pixels, ke[0], ke[1], ke[2], d["rounds"],
                100.0 * d["skipped_rounds"] / d["rounds"] if d["rounds"] else 0.0,
                100.0 * d["llf_only"][0] / d["waves"], 100.0 * d["llf_only"][2] / d["waves"], d["waves"]))
        print("prefetching classes: %.1f%% of the staging rounds reach no coefficient; frame: sum of kend = %.1f%% of all positions\n" % (
            100.0 * tot_skipped / max(tot_rounds, 1), 100.0 * tot_kend / (3 * pixels)))


if __name__ == "__main__":
    main()
