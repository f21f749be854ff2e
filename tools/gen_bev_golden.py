"""Writes tests/golden/bev_recorded_run.npz from a run the reference recorded itself (its
kuruma/test/output directory): the car position of ..._control_data.json and the centreline of
..._path_data.json, both in world centimetres.

    python tools/gen_bev_golden.py REFERENCE/kuruma/test/output [raw_20250702_024355_405]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def find(node, key):
    if isinstance(node, dict):
        if key in node:
            return node[key]
        node = list(node.values())
    if isinstance(node, list):
        for v in node:
            got = find(v, key)
            if got is not None:
                return got
    return None


def main(out_dir, stem="raw_20250702_024355_405"):
    with open(os.path.join(out_dir, stem + "_control_data.json")) as f:
        car = find(json.load(f), "car_position")
    with open(os.path.join(out_dir, stem + "_path_data.json")) as f:
        line = json.load(f)["centerline_world"]
    np.savez(os.path.join(ROOT, "tests", "golden", "bev_recorded_run.npz"),
             car_position=np.array(car, dtype=np.float64),
             centerline_world=np.array(line, dtype=np.float64),
             source=np.array(stem))


if __name__ == "__main__":
    main(*sys.argv[1:])
