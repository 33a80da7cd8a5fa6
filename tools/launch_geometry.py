"""Launch geometry per kernel from a `rocprofv3 --kernel-trace` CSV: for every kernel name the number of launches with each
(grid, workgroup, LDS bytes) it was launched with. Two libraries that launch the same work give the same table.
  python tools/launch_geometry.py TRACE.csv > geometry.csv
  python tools/launch_geometry.py --compare PARENT_TRACE.csv BRANCH_TRACE.csv [--only SUBSTRING ...]
--only keeps the kernels whose name holds one of the substrings (the kernels of the sources under comparison)."""
import collections
import csv
import sys


def geometry(path):
    """{(kernel name, grid xyz, workgroup xyz, LDS bytes): launches}"""
    out = collections.Counter()
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
            wg = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
            out[(r["Kernel_Name"], grid, wg, r["LDS_Block_Size"])] += 1
    return out


def rows(g):
    return [(k[0], n, k[1], k[2], k[3]) for k, n in sorted(g.items())]


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--compare":
        only = args[args.index("--only") + 1:] if "--only" in args else []
        keep = lambda g: {k: n for k, n in g.items() if not only or any(s in k[0] for s in only)}
        a, b = keep(geometry(args[1])), keep(geometry(args[2]))
        diff = sorted(k for k in set(a) | set(b) if a.get(k, 0) != b.get(k, 0))
        for k in diff:
            print(f"DIFFERENT {k}: parent {a.get(k, 0)} launches, branch {b.get(k, 0)}")
        names = {k[0] for k in a}
        print(f"{len(names)} kernels, {len(a)} (kernel, grid, workgroup, LDS) rows, {sum(a.values())} launches in the parent's trace; "
              f"{len(diff)} rows differ")
        sys.exit(1 if diff else 0)
    w = csv.writer(sys.stdout)
    w.writerow(["Name", "Calls", "Grid", "Workgroup", "LDS"])
    w.writerows(rows(geometry(args[0])))
