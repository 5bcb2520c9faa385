#!/usr/bin/env python3
"""Writes tests/golden/own_tree_gpu_digests.json: the digests tests/test_gpu_own_tree_builder.py::test_device_image_is_the_recorded_one
compares (the cases are listed there). Needs the GPU.

    python tests/golden/make_own_tree_gpu_digests.py

Run it on a build whose device trees are known to be right: it records what the library builds, whatever that is.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "wgpu-path-tracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ptmi import native  # noqa: E402
import test_gpu_own_tree_builder as T  # noqa: E402


def main():
    out = {}
    with native.Context(0) as ctx:
        ctx.set_options(leaves=2, leaf_tris=0, keep_reference_tree=0, tree_builder=2, traversal=native.TRAVERSAL_AUTO, cull=1)
        for name, leaf_tris in T.DIGEST_CASES:
            st, d = T.device_image_digests(ctx, name, leaf_tris)
            if st.tree_builder_used != 2:
                raise SystemExit(f"{name}, leaf_tris {leaf_tris}: the device builder did not run (tree_builder_used {st.tree_builder_used})")
            out[T.digest_key(name, leaf_tris)] = d
            print(T.digest_key(name, leaf_tris), d["wnodes"][:16], "quantised" if d["qnodes"] else "not quantised")
    with open(T.DIGESTS, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
