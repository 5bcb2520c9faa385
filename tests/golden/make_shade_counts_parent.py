#!/usr/bin/env python3
"""tests/golden/make_shade_counts_parent.py <commit> [out.json]: writes shade_counts_parent.json from the build that PTMI_LIB names, which
is to be the parent commit's libptmi.so (the commit before `shade`'s statistics moved into the compaction): the counters
tests/test_gpu_shade_counts.py compares this build's with. Needs the GPU."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "wgpu-path-tracing_amd"), os.path.dirname(HERE)):
    sys.path.insert(0, p)


def main(commit, out=os.path.join(HERE, "shade_counts_parent.json")):
    from ptmi import native, scenes
    import test_gpu_shade_counts as T
    assert os.environ.get("PTMI_LIB"), "PTMI_LIB must name the parent build's libptmi.so"
    with native.Context(0) as c:
        rec = T.RECORD(c, scenes.make("cornell"), commit)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main(*sys.argv[1:])
