"""Reduces a rocprofv3 --kernel-trace CSV (…_kernel_trace.csv) to the ordered list of kernel launches.  A launch is (kernel name
without its parameter list, grid, workgroup, LDS bytes); the output names every distinct launch once (`k7 = name | grid | wg | lds`, in
order of first appearance) and then gives the sequence in start order as those ids, `k7x3` for three in a row.  The runtime's own copy
and fill kernels (__amd_rocclr_*: what hipMemcpy and hipMemset turn into) are left out — they are not launches of the library.  Two runs
of the same program launched the same kernels when their outputs are equal.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python scripts/launch_paths.py --per-agent
    python scripts/launch_trace_list.py DIR/<host>/kt_kernel_trace.csv > launches.txt

With --calls CASES.json (what scripts/fe_launch_paths.py --out wrote under the same trace) the trace is cut into that table's calls:
the script launched a delimiter — nep::gjk_explicit_kernel over 64 n work-items, n = 1, 2, ... — in front of every call and behind
it.  Every delimiter must be there once and in order; they are dropped, and so is whatever ran between two calls (a handle's set-up)
and every kernel that is not the library's.  The output gives the distinct launches as above and one line of ids per call;
--fixture OUT writes the table with those lines added.

    python scripts/launch_trace_list.py --calls CASES.json DIR/<host>/kt_kernel_trace.csv --fixture tests/golden/fe_launch_paths.json
"""
import csv
import json
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


DELIMITER = "nep::gjk_explicit_kernel"


def by_call(seq):
    """the library's launches between delimiter 2c + 1 and 2c + 2, for c = 0, 1, ... -> [[launch]]"""
    calls, n, cur = [], 0, None
    for line in seq:
        name, grid = [w.strip() for w in line.split("|")[:2]]
        if name == DELIMITER:
            n += 1
            if int(grid.split("x")[0]) != 64 * n:
                raise SystemExit("delimiter %d missing or out of order: %s" % (n, line))
            if n % 2:
                cur = []
            else:
                calls.append(cur); cur = None
        elif cur is not None and "nep::" in name:
            cur.append(line)
    if cur is not None:
        raise SystemExit("the trace ends inside a call")
    return calls


def main(argv):
    if "--calls" not in argv:
        write(launches(argv[0]))
        return
    argv = list(argv)
    fixture = argv.pop(argv.index("--fixture") + 1) if "--fixture" in argv else None
    table = argv.pop(argv.index("--calls") + 1)
    trace = [a for a in argv if not a.startswith("--")][0]
    with open(table) as f:
        doc = json.load(f)
    calls = by_call(launches(trace))
    if len(calls) != sum(len(c["calls"]) for c in doc["cases"]):
        raise SystemExit("%d calls in the trace, %d in the table" % (len(calls), sum(len(c["calls"]) for c in doc["cases"])))
    ids, it = {}, iter(calls)
    for c in doc["cases"]:
        for call in c["calls"]:
            call["launches"] = " ".join("k%d" % ids.setdefault(line, len(ids)) for line in next(it))
    doc["launch_ids"] = {"k%d" % k: line for line, k in ids.items()}
    for k, line in doc["launch_ids"].items():
        sys.stdout.write("%s = %s\n" % (k, line))
    sys.stdout.write("\n")
    for c in doc["cases"]:
        for r, call in enumerate(c["calls"]):
            sys.stdout.write("%s %d x %d, call %d: %s\n" % (c["name"], c["scenes"], c["agents"], r, call["launches"]))
    if fixture:
        sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.abspath(__file__)))
        from fe_launch_paths import write_fixture
        with open(fixture, "w") as f:
            write_fixture(doc, f)


if __name__ == "__main__":
    main(sys.argv[1:])
