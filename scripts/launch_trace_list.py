"""Reduces a rocprofv3 --kernel-trace CSV (…_kernel_trace.csv) to the ordered list of kernel launches.  A launch is (kernel name
without its parameter list, grid, workgroup, LDS bytes); the output names every distinct launch once (`k7 = name | grid | wg | lds`, in
order of first appearance) and then gives the sequence in start order as those ids, `k7x3` for three in a row.  The runtime's own copy
and fill kernels (__amd_rocclr_*: what hipMemcpy and hipMemset turn into) are left out — they are not launches of the library.  Two runs
of the same program launched the same kernels when their outputs are equal.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python scripts/launch_paths.py --per-agent
    python scripts/launch_trace_list.py DIR/<host>/kt_kernel_trace.csv > launches.txt
"""
import csv
import sys


def short(name):
    """the kernel's name without its parameter list (template arguments stay)"""
    name = name.strip()
    if not name.endswith(")"):
        return name
    depth = 0
    for i in range(len(name) - 1, -1, -1):
        depth += (name[i] == ")") - (name[i] == "(")
        if depth == 0:
            return name[:i].strip()
    return name


def launches(path):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id", 0))))
    for r in rows:
        if r["Kernel_Name"].startswith("__amd_rocclr_"):
            continue
        grid = "x".join(r[k] for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z") if k in r) or r.get("Grid_Size", "?")
        wg = "x".join(r[k] for k in ("Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z") if k in r) or r.get("Workgroup_Size", "?")
        yield "%s | %s | %s | %s" % (short(r["Kernel_Name"]), grid, wg, r.get("LDS_Block_Size", "?"))


def write(seq, out=sys.stdout):
    ids, runs = {}, []
    for line in seq:
        k = ids.setdefault(line, len(ids))
        if runs and runs[-1][0] == k:
            runs[-1][1] += 1
        else:
            runs.append([k, 1])
    for line, k in ids.items():
        out.write("k%d = %s\n" % (k, line))
    out.write("\n")
    words = ["k%d" % k if n == 1 else "k%dx%d" % (k, n) for k, n in runs]
    for i in range(0, len(words), 24):
        out.write(" ".join(words[i:i + 24]) + "\n")


if __name__ == "__main__":
    write(launches(sys.argv[1]))
