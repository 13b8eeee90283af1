"""scripts/host_entry_time.py on two builds of the library, alternating: RUNS runs of the pair (one fresh process per library and run; the order of the two
processes changes from run to run), and after them a control, the OTHER library twice in a row, which shows what two processes of one and the same library differ
by. The rule, per run: this tree's median lies within the other library's [min, max] of the same run. Writes every call's time and the rule's outcome.
usage: python scripts/host_entry_compare.py OTHER_LIB.so [OUT.json]   (default: profiles/batch_refactor_host_entry.json; HEC_RUNS, default 3)"""
import json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER = os.path.abspath(sys.argv[1])
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "batch_refactor_host_entry.json")
RUNS = int(os.environ.get("HEC_RUNS", "3"))


def one(lib):
    """one process of host_entry_time.py against `lib` (None: this tree's library) -> its row"""
    env = dict(os.environ)
    env.pop("MBLS_LIB", None)
    if lib:
        env["MBLS_LIB"] = lib
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "row.json")
        subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "host_entry_time.py"), "row", f], env=env, check=True, timeout=300, stdout=subprocess.DEVNULL)
        with open(f) as fh:
            return json.load(fh)["row"]


def judge(ref, new):
    return {"median_within_reference_min_max": bool(ref["ms_min"] <= new["ms_median"] <= ref["ms_max"]),
            "median_minus_reference_median_ms": round(new["ms_median"] - ref["ms_median"], 3)}


runs = []
for r in range(RUNS):
    order = ["parent", "this_tree"] if r % 2 == 0 else ["this_tree", "parent"]
    rows = {}
    for which in order:
        rows[which] = one(OTHER if which == "parent" else None)
    run = {"process_order": order, "parent": rows["parent"], "this_tree": rows["this_tree"]}
    run.update(judge(rows["parent"], rows["this_tree"]))
    runs.append(run)
    print("run %d %s: parent %.3f [%.3f, %.3f]   this tree %.3f   within: %s" % (r, order, rows["parent"]["ms_median"], rows["parent"]["ms_min"], rows["parent"]["ms_max"],
                                                                              rows["this_tree"]["ms_median"], run["median_within_reference_min_max"]), flush=True)
first, second = one(OTHER), one(OTHER)
control = {"what": "the parent's library twice in a row: the second process judged against the first by the same rule", "first": first, "second": second}
control.update(judge(first, second))
print("control: first %.3f [%.3f, %.3f]   second %.3f   within: %s" % (first["ms_median"], first["ms_min"], first["ms_max"], second["ms_median"],
                                                                       control["median_within_reference_min_max"]), flush=True)
out = {"what": "one host call of mbls_fast_aggregate_verify_batch, 2^16 items x 128 96-byte keys in pageable host memory (scripts/host_entry_time.py): one warm-up "
               "call and five timed calls per process, one process per library and run (scripts/host_entry_compare.py)",
       "rule": "per run: this tree's median within the parent's [min, max] of the same run",
       "runs": runs, "runs_within": sum(r["median_within_reference_min_max"] for r in runs), "runs_total": len(runs), "control": control}
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print("wrote", OUT)
