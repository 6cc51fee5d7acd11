#!/usr/bin/env python3
"""Compares one of the raster timing tools (raster_ms.py, raster_tex_ms.py, raster_bc1_ms.py) run on the parent commit's library and
on this commit's: reads the --out files of the runs (run alternately in one session: PBR_HIP_LIB points a run at the parent's
library) and prints, per row of the tool's table, the runs' raster ms, the parent's own max - min, the difference of the medians and
whether it lies within that spread.  --profile F writes profile F: the first of --this-runs (the tool's own output for this commit),
what --keep names of the old profile from its first line starting with that text on (an earlier comparison), and this table.
Usage: python tools/raster_ab_table.py --tool tools/raster_ms.py --what "..." --parent-runs P1 P2 P3 --this-runs T1 T2 T3
       [--profile profiles/raster_ms.txt [--keep "existing path"]]"""
import argparse
import re
import statistics


def rows(path):
    """{(row name, size): raster ms} of one output file: the lines that hold `<name>  <w>x<h>  <triangles>  <raster ms> ...`"""
    out = {}
    for line in open(path):
        m = re.match(r"^(\S.*?)\s+(\d+x\d+)\s+(\d+)\s+(\d+\.\d+)\s", line)
        if m:
            out[(m.group(1), m.group(2))] = float(m.group(4))
    return out


def table(tool, what, parent_files, this_files):
    parent, this = [rows(p) for p in parent_files], [rows(p) for p in this_files]
    lines = ["", f"{what}: {tool} on the parent commit's library and on this commit's, run alternately in one session "
             f"({len(parent)} + {len(this)} runs), raster ms:",
             f"{'row':<30}{'size':>11}  {'parent runs':<26}{'this commit runs':<26}{'parent max-min':>15}{'median diff':>13}  verdict"]
    for key in parent[0]:
        p, t = [r[key] for r in parent], [r[key] for r in this]
        spread, diff = max(p) - min(p), statistics.median(t) - statistics.median(p)
        lines.append(f"{key[0]:<30}{key[1]:>11}  {' '.join(f'{x:.4f}' for x in p):<26}{' '.join(f'{x:.4f}' for x in t):<26}{spread:>15.4f}"
                     f"{diff:>+13.4f}  " + ("within the spread" if diff <= spread else f"slower by {100 * diff / statistics.median(p):.1f} %"))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tool", required=True)
    ap.add_argument("--what", default="this commit against its parent")
    ap.add_argument("--parent-runs", nargs="+", required=True)
    ap.add_argument("--this-runs", nargs="+", required=True)
    ap.add_argument("--profile")
    ap.add_argument("--keep")
    a = ap.parse_args()
    lines = table(a.tool, a.what, a.parent_runs, a.this_runs)
    print("\n".join(lines))
    if a.profile:
        kept = []
        if a.keep:
            old = open(a.profile).read().split("\n")
            start = next((i for i, l in enumerate(old) if l.startswith(a.keep)), None)
            if start is not None:
                kept = [""] + [l for l in old[start:] if l]
        body = open(a.this_runs[0]).read().rstrip("\n").split("\n")
        while body and not body[-1]:
            body.pop()
        open(a.profile, "w").write("\n".join(body + kept + lines) + "\n")


if __name__ == "__main__":
    main()
