#!/usr/bin/env python3
"""Writes tests/golden/image_digests.json: the digests tests/test_image_digests_host.py compares (the cases are listed there).

    python tests/golden/make_image_digests.py

Run it on a build whose images are known to be right: it records what the library builds, whatever that is.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "wgpu-path-tracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_image_digests_host as T  # noqa: E402


def main():
    images = {}
    for name, leaves, leaf_tris in T.CASES:
        d, info = T.image_digests(name, leaves, leaf_tris)
        images[T.key(name, leaves, leaf_tris)] = d
        print(T.key(name, leaves, leaf_tris), info.n_wnodes, "wide nodes, quantised", info.quantised)
    stats = {name: T.stats_values(name) for name in T.STATS}
    with open(T.GOLDEN, "w") as f:
        json.dump({"images": images, "stats": stats}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
