"""Generate tests/golden/federated_splits/ by RUNNING the reference's class-shard splitter.

Build container only (the reference never travels).  Loads src/datasets/federated_split.py by
file path (an installed `datasets` package shadows the reference's folder on sys.path) and runs
`make_class_shard_splits` on a 228-line base split of 12 classes -- 6 + 5 (c mod 4) + c lines
for class c, shuffled with random.Random(7) -- for the four cases below.  Output is data only:
base.txt, and per case the client split files and the returned stats (stats.json).

    python tests/golden/make_golden_federated.py <reference root>
"""
import importlib.util
import json
import os
import random
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "federated_splits")
# (clients, shards_per_client, min_samples_per_client, seed)
CASES = [(4, 3, 10, 42), (4, 2, 40, 42), (5, 1, 30, 42), (3, 6, 200, 42)]


def case_name(clients, shards, min_samples, seed):
    return f"c{clients}_s{shards}_m{min_samples}_seed{seed}"


def base_lines():
    lines = [f"videos/class{c:02d}/clip_{i:03d} {c}" for c in range(12) for i in range(6 + 5 * (c % 4) + c)]
    random.Random(7).shuffle(lines)
    return lines


def main():
    ref_root = sys.argv[1]
    spec = importlib.util.spec_from_file_location(
        "ref_federated_split", os.path.join(ref_root, "src", "datasets", "federated_split.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    base = os.path.join(OUT, "base.txt")
    with open(base, "w", encoding="utf-8") as f:
        f.write("\n".join(base_lines()) + "\n")
    for clients, shards, min_samples, seed in CASES:
        dst = os.path.join(OUT, case_name(clients, shards, min_samples, seed))
        os.makedirs(dst)
        with tempfile.TemporaryDirectory() as tmp:
            paths, stats = ref.make_class_shard_splits(base, clients, shards_per_client=shards, seed=seed,
                                                       min_samples_per_client=min_samples, out_prefix="fed",
                                                       out_dir=tmp)
            for i, p in enumerate(paths):
                assert os.path.basename(p) == f"fed_client_{i}_train.txt"
                shutil.copy(p, os.path.join(dst, f"client_{i}.txt"))
        with open(os.path.join(dst, "stats.json"), "w", encoding="utf-8") as f:
            json.dump(stats, f, indent=1)
        print(case_name(clients, shards, min_samples, seed), [s["num_samples"] for s in stats])


if __name__ == "__main__":
    main()
