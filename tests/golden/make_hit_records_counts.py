"""Executed-test counts of the one-hit fused plan's counting instantiations on the seeded scenes of
tests/test_hit_records_gpu.py (COUNT_SCENES), written to hit_records_exec_counts.json.

Run on an MI355X with the build whose counts are the reference, from the repository root:
    ART_LIB=<that build's libart.so> python tests/golden/make_hit_records_counts.py
The committed file was taken on the commit before the cast handed over hit records (every consumer
rebuilt the hit from the nearest-hit record); the records must not change a single executed test.
Each scene runs twice and the two counts must agree.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "audio-raytracer_amd"), os.path.join(ROOT, "tests")]

import art  # noqa: E402
import test_hit_records_gpu as t  # noqa: E402


def main():
    out = {}
    with art.Context(1) as ctx:
        for name in t.COUNT_SCENES:
            scene, org = t.count_scene(name)
            a, b = (t.executed_counts(ctx, scene, org)[2] for _ in range(2))
            assert a == b, f"{name}: the counts differ between two runs"
            out[name] = a
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "hit_records_exec_counts.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
