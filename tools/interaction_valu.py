#!/usr/bin/env python3
"""VALU instructions of rsv_witness_interaction_dev per accepted proof, for tools/bench_interaction.py's roofline bound.

    rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d OUT -o pmc -- python3 tools/bench_interaction.py ... > OUT/bench.json
    python tools/interaction_valu.py TAG OUT/pmc_counter_collection.csv OUT/bench.json [more CSV / JSON pairs]

Takes the last dispatch of each interaction kernel in each pass (wave-level instructions), divides by the pass's accepted
proofs and writes profiles/interaction_valu.json: per shape "log_plonk/log_poseidon", keyed by the hash of the kernel
sources (a pass on other sources is refused)."""
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    tag, pairs = sys.argv[1], sys.argv[2:]
    out = {"tag": tag, "kernel_sources_sha": bench.kernel_sources_sha(), "unit": "wave64 VALU instructions per accepted proof",
           "shapes": {}}
    for path, bjson in zip(pairs[0::2], pairs[1::2]):
        with open(bjson) as f:
            b = json.loads(f.read().strip().splitlines()[-1])
        if b["kernel_sources_sha"] != out["kernel_sources_sha"]:
            raise SystemExit(f"{bjson}: other kernel sources")
        per = {}
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"].split("(")[0].replace("void ", "")
                if "k_int_" not in name or r["Counter_Name"] != "SQ_INSTS_VALU":
                    continue
                d = per.setdefault(name, {})
                d[int(r["Dispatch_Id"])] = d.get(int(r["Dispatch_Id"]), 0.0) + float(r["Counter_Value"])
        cfg = b["config"]
        accepted = cfg["proofs"] - cfg["rejected"]
        out["shapes"][f"{cfg['log_plonk']}/{cfg['log_poseidon']}"] = {
            "kernels": {k: v[max(v)] / accepted for k, v in sorted(per.items())},
            "total": sum(v[max(v)] for v in per.values()) / accepted, "proofs": cfg["proofs"], "accepted": accepted}
    with open(os.path.join(ROOT, "profiles", "interaction_valu.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
